"""TEST INFRASTRUCTURE.  A NumPy restatement of the learner state blob (include/crowdnav.h: cn_state_header, cn_state_segment,
cn_td3_state_*, cn_td3_pop_state_*): which segments a TD3 handle or population has, where they lie, and the bytes of a blob packed
from given tensors.  Written from the header's statement alone; it shares no code with csrc/crowdnav_state.hip."""
import struct

import numpy as np

MAGIC, VERSION, FAMILY_TD3 = 0x0045544154534E43, 1, 1
PARAM, MOMENT, ADAM, STEPS, PW, COUNTER, LOSS, HYPER, PBT, PBT_LAST = range(10)
HEADER = struct.Struct("<Q8iQ")         # magic; version, family, n_members, obs_dim, hidden, batch, pbt_bound, n_segments; total_bytes
SEGMENT = struct.Struct("<4i2Q")        # member, kind, index, reserved; offset, bytes
HEADER_FIELDS = ("magic", "version", "family", "n_members", "obs_dim", "hidden", "batch", "pbt_bound", "n_segments", "total_bytes")
PBT_STATE_BYTES = 16 + 64 * 32          # cn_td3_pbt_state
HYPERS = 5


def round16(x):
    return (x + 15) // 16 * 16


def param_words(obs_dim, hidden, net_in, net_out):
    """Words of w1, b1, w2, b2, w3, b3 of Linear(net_in, H) - Linear(H, H) - Linear(H, net_out)."""
    h = hidden
    return [h * net_in, h, h * h, h, net_out * h, net_out]


def member_segments(p, obs_dim, hidden, population):
    """(member, kind, index, bytes) of member p, in the blob's order."""
    actor, critic = param_words(obs_dim, hidden, obs_dim, 2), param_words(obs_dim, hidden, obs_dim + 2, 1)
    out = []
    for net, words in enumerate((actor, actor, critic, critic, critic, critic)):          # actor, actor_t, q1, q1_t, q2, q2_t
        out += [(p, PARAM, net * 6 + j, 4 * w) for j, w in enumerate(words)]
    for net, words in enumerate((actor, critic, critic)):                                  # the optimised networks, (m, v) per tensor
        out += [(p, MOMENT, (net * 6 + j) * 2 + k, 4 * w) for j, w in enumerate(words) for k in range(2)]
    out += [(p, ADAM, 0, 16), (p, STEPS, 0, 8), (p, PW, 0, 32), (p, COUNTER, 0, 8), (p, LOSS, 0, 4)]
    if population:
        out.append((p, HYPER, 0, 4 * HYPERS))
    return out


def segments(P, obs_dim, hidden, pbt_bound=False, population=None):
    population = bool(population)           # a cn_td3_pop handle (any P) has the hyper-parameter segments; a solo handle has not
    out = []
    for p in range(P):
        out += member_segments(p, obs_dim, hidden, population)
    if pbt_bound:
        out += [(-1, PBT, 0, PBT_STATE_BYTES), (-1, PBT_LAST, 0, 16 * P)]
    return out


def directory(P, obs_dim, hidden, batch, pbt_bound=False, population=None):
    """-> (header dict, [(member, kind, index, offset, bytes)], total_bytes)."""
    segs = segments(P, obs_dim, hidden, pbt_bound, population)
    off = HEADER.size + SEGMENT.size * len(segs)
    rows = []
    for m, k, i, nb in segs:
        rows.append((m, k, i, off, nb))
        off += round16(nb)
    header = dict(magic=MAGIC, version=VERSION, family=FAMILY_TD3, n_members=P, obs_dim=obs_dim, hidden=hidden, batch=batch,
                  pbt_bound=int(bool(pbt_bound)), n_segments=len(segs), total_bytes=off)
    return header, rows, off


def total_bytes(P, obs_dim, hidden, pbt_bound=False, population=None):
    """The formula: header + directory + every segment rounded up to 16 bytes."""
    population = bool(population)           # a cn_td3_pop handle (any P) has the hyper-parameter segments; a solo handle has not
    D, H = obs_dim, hidden
    actor = [H * D, H, H * H, H, 2 * H, 2]
    critic = [H * (D + 2), H, H * H, H, H, 1]
    r = lambda words: sum(round16(4 * w) for w in words)
    member = 2 * r(actor) + 4 * r(critic) + 2 * (r(actor) + 2 * r(critic)) + 16 + 16 + 32 + 16 + 16 + (32 if population else 0)
    nseg = P * (36 + 36 + 5 + (1 if population else 0)) + (2 if pbt_bound else 0)
    return 48 + 32 * nseg + P * member + ((round16(PBT_STATE_BYTES) + round16(16 * P)) if pbt_bound else 0)


def pack(P, obs_dim, hidden, batch, tensors, pbt_bound=False, population=None):
    """The blob's bytes (uint8 array) from `tensors`: one array per segment in directory order, of exactly the segment's bytes."""
    header, rows, total = directory(P, obs_dim, hidden, batch, pbt_bound, population)
    assert len(tensors) == len(rows)
    blob = np.zeros(total, dtype=np.uint8)
    blob[:HEADER.size] = np.frombuffer(HEADER.pack(*[header[k] for k in HEADER_FIELDS]), dtype=np.uint8)
    at = HEADER.size
    for m, k, i, off, nb in rows:
        blob[at:at + SEGMENT.size] = np.frombuffer(SEGMENT.pack(m, k, i, 0, off, nb), dtype=np.uint8)
        at += SEGMENT.size
    for (m, k, i, off, nb), t in zip(rows, tensors):
        b = np.ascontiguousarray(t).view(np.uint8).reshape(-1)
        assert b.size == nb, (m, k, i, b.size, nb)
        blob[off:off + nb] = b
    return blob


def unpack(blob):
    """-> (header dict, [(member, kind, index, offset, bytes)]) as the blob's own header and directory say."""
    b = np.ascontiguousarray(blob).view(np.uint8).tobytes()
    header = dict(zip(HEADER_FIELDS, HEADER.unpack_from(b, 0)))
    rows = []
    for s in range(header["n_segments"]):
        m, k, i, _, off, nb = SEGMENT.unpack_from(b, HEADER.size + s * SEGMENT.size)
        rows.append((m, k, i, off, nb))
    return header, rows
