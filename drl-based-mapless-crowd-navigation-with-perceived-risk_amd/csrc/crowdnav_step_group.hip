// crowdnav_step_group.hip -- the compile unit of the group kernels (CN_GROUP_KERNELS, crowdnav_variants.h): cn_step_group_*'s one launch
// for J handles.  Their definitions are the group-only section of crowdnav_kernel.hip, next to the step body they instantiate; this file
// selects that section -- none of the kernel file's units 1-5 -- and includes it, so unit 1's compile stays what it is.
#define CN_STEP_GROUP_UNIT 1
#define CN_TU 0
#include "crowdnav_kernel.hip"
