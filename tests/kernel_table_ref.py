"""The kernel selection of libcrowdnav.so written out as data, independently of csrc/crowdnav_variants.h: which world (class of
configurations cn_create accepts) launches which kernel for which call, the rules of the plain tracker worlds' step geometry, and
the compile unit (csrc/build.sh, CN_TU) of every kernel.  tests/test_kernel_table.py holds the header's pure selection function
to it on the CPU, tests/test_gpu_kernel_table.py a live handle of every world."""

# world: (facts, step, same-call reset, external, sequence, policy).  facts = the arguments of cn_world_index:
# (obs_layout, wide, gt, wheel ramp, dense social force, social force, contact ticks, shape360, shape720).
# External: every layout-0 tracker world that is not wide gets cn_env_kernel_ext; every gt world none.
# The step kernel of the three plain tracker worlds is the oldest-first, one-wave-per-workgroup one here; want_step() has the rest.
E, S = "cn_env_kernel", "cn_policy_kernel"
WORLDS = {
    "rw":      ((2, 0, 0, 0, 0, 0, 0, 0, 0), E + "_rw", E + "_rw_same", E + "_rw_ext", E + "_seq_rw", S + "_rw"),
    "orig":    ((1, 0, 0, 0, 0, 0, 0, 0, 0), E + "_orig", E + "_orig_same", E + "_orig_ext", E + "_seq_orig", S + "_orig"),
    "wide":    ((0, 1, 0, 0, 0, 0, 0, 0, 0), E + "_wide", E + "_wide_same", E + "_wide_ext", E + "_seq_wide", S + "_wide"),
    "wa":      ((0, 0, 0, 1, 0, 0, 0, 0, 0), E + "_wa", E + "_wa_same", E + "_ext", E + "_seq_wa", S + "_wa"),
    "gt_wa":   ((0, 0, 1, 1, 0, 0, 0, 0, 0), E + "_gt_wa", E + "_gt_wa_same", None, E + "_gt_seq_wa", S + "_gt_wa"),
    "sfd":     ((0, 0, 0, 0, 1, 1, 0, 0, 0), E + "_sfd", E + "_sfd_same", E + "_ext", E + "_seq_sfd", S + "_sfd"),
    "gt_sfd":  ((0, 0, 1, 0, 1, 1, 0, 0, 0), E + "_gt_sfd", E + "_gt_sfd_same", None, E + "_gt_seq_sfd", S + "_gt_sfd"),
    "sf":      ((0, 0, 0, 0, 0, 1, 0, 0, 0), E + "_sf", E + "_sf_same", E + "_ext", E + "_seq_sf", S + "_sf"),
    "gt_sf":   ((0, 0, 1, 0, 0, 1, 0, 0, 0), E + "_gt_sf", E + "_gt_sf_same", None, E + "_gt_seq_sf", S + "_gt_sf"),
    "ct":      ((0, 0, 0, 0, 0, 0, 1, 0, 0), E + "_ct", E + "_ct_same", E + "_ext", E + "_seq_ct", S + "_ct"),
    "gt_ct":   ((0, 0, 1, 0, 0, 0, 1, 0, 0), E + "_gt_ct", E + "_gt_ct_same", None, E + "_gt_seq_ct", S + "_gt_ct"),
    "gt":      ((0, 0, 1, 0, 0, 0, 0, 0, 0), E + "_gt", E + "_gt_same", None, E + "_gt_seq", S + "_gt"),
    "generic": ((0, 0, 0, 0, 0, 0, 0, 0, 0), E, E + "_same", E + "_ext", E + "_seq", S),
    "s360":    ((0, 0, 0, 0, 0, 0, 0, 1, 0), E + "_s360", E + "_same", E + "_ext", E + "_seq_s360", S + "_s360"),
    "s720":    ((0, 0, 0, 0, 0, 0, 0, 0, 1), E + "_s720", E + "_same", E + "_ext", E + "_seq_s720", S + "_s720"),
}
PLAIN_TRACKER = ("generic", "s360", "s720")
HEADLINE_ONLY = [E + "_fair", E + "_fair_s360", E + "_s360_w4", E + "_fair_s360_w4", E + "_s360_x2", E + "_fair_s720"]
ARB_AUTO, ARB_OLDEST_FIRST, ARB_FAIR = 0, 1, 2


def want_step(world, arbitration, overlapped, n_cus, n_envs, group_envs, x2, wpb):
    """The step kernel of a launch.  Fair: arbitration fair, or auto with a launch that is not overlapped and fills the device on
    its own (n_envs >= 8 per CU); only the plain tracker worlds have fair forms.  The 360-ray shape, with resident = max(n_envs,
    group_envs) and a known CU count: two waves per environment if CN_X2=1, or unset and resident <= 8 per CU; else four
    environments per workgroup if CN_WPB is not off and resident <= 16 per CU; else one wave per workgroup."""
    base = WORLDS[world][1]
    if world not in PLAIN_TRACKER:
        return base
    fair = arbitration == ARB_FAIR or (arbitration == ARB_AUTO and not overlapped and n_cus > 0 and n_envs >= 8 * n_cus)
    if world == "s360" and n_cus > 0:
        resident = max(n_envs, group_envs)
        if x2 == 1 or (x2 < 0 and resident <= 8 * n_cus):
            return E + "_s360_x2"
        if wpb != 0 and resident <= 16 * n_cus:
            return E + ("_fair_s360_w4" if fair else "_s360_w4")
    return base.replace(E, E + "_fair", 1) if fair else base


# the compile unit of every kernel: unit 1 has every one-step kernel, units 2-5 the sequence and policy kernels
UNIT = {}
for _w in WORLDS.values():
    for _n in _w[1:4]:
        if _n:
            UNIT[_n] = 1
for _n in HEADLINE_ONLY:
    UNIT[_n] = 1
for _u, _names in {
    2: [E + "_seq", E + "_seq_s360", E + "_seq_s720", E + "_gt_seq", E + "_seq_wide", S, S + "_s360", S + "_gt", S + "_wide"],
    3: [E + "_seq_sf", E + "_seq_sfd", E + "_seq_wa", E + "_gt_seq_sf", E + "_gt_seq_sfd", E + "_gt_seq_wa"],
    4: [S + "_s720", S + "_sf", S + "_sfd", S + "_wa", S + "_gt_sf", S + "_gt_sfd", S + "_gt_wa"],
    5: [E + "_seq_ct", E + "_gt_seq_ct", E + "_seq_orig", E + "_seq_rw", S + "_ct", S + "_gt_ct", S + "_orig", S + "_rw"],
}.items():
    for _n in _names:
        UNIT[_n] = _u
assert len(UNIT) == 68
