// crowdnav_state.h -- what crowdnav_state.hip (a learner's state as one blob: cn_td3_state_*, cn_td3_pop_state_*; the statement is
// include/crowdnav.h's) asks of the unit that owns a handle: the list of its live state, in the blob's segment order.  Host code.
// A family joins by writing one such list (crowdnav_td3.hip: td3_state_view, td3_pop_state_view); the blob, the job table and the
// kernel do not know the families apart.
#pragma once
#include <stdint.h>
#include <vector>

#include "../../include/crowdnav.h"

#pragma GCC visibility push(hidden)

struct StateSeg { void* live; int32_t member, kind, index; uint32_t words; };     // `words` 4-byte words at `live` (null: CN_STATE_HYPER)
// hyper-parameter `hyper` of `member` lies at `live` too: the load writes every one, the save reads the first of each (member, hyper)
struct StateScatter { float* live; int32_t member, hyper; };
struct StateTable;                                 // crowdnav_state.hip: the device job table, the header and directory as they go out
void state_table_free(StateTable* t);
struct StateView {
    int family = 0, P = 0, obs_dim = 0, hidden = 0, batch = 0, pbt_bound = 0, device = 0;
    StateTable** table = nullptr;                  // the handle's slot for the table built from this view
    std::vector<StateSeg> seg;                     // (filled only when `full`)
    std::vector<StateScatter> scatter;
};
void td3_state_view(cn_td3_handle h, bool full, StateView& v);
void td3_pop_state_view(cn_td3_pop_handle h, bool full, StateView& v);

#pragma GCC visibility pop
