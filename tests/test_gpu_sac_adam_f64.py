"""cn_sac_update's Adam across four updates against the float64 series of tests/sac_f64.py (adam_series.run): the tick's step count
and three bias-correction pairs, the moments of Q, V, the actor's trunk and its two head jobs, and V's soft update in both
soft_update modes, observed through every weight read back before and after every update; then a new handle on the stepped
parameters (fresh state at create).  Each wrong restatement of the series (sac_f64.SERIES_VARIANTS) must be rejected on the
network it concerns; a log_std output clamped on every row and a planted dead unit of Q must keep every bit of their weights.
tests/test_sac_f64_helpers.py runs the same cases on the CPU with the kernel's formula emulated in float32.
`-s` prints the worst error / bound per network and update and every variant's ratios."""
import pytest

import adam_series as A
import sac_f64 as S
from learner_handle import LearnerHandle, batch_struct

pytestmark = pytest.mark.gpu


class Handle(LearnerHandle):
    """adam_series.run's learner: one cn_sac handle; write() copies into the tensors whose pointers the handle holds."""

    def __init__(self, P, shape, hp):
        self.P = {n: {k: v.detach().clone().float().cuda().contiguous() for k, v in p.items()} for n, p in P.items()}
        cfg = S.handle_config(self.P, shape, soft_update=hp["soft_update"], tau=hp["tau"], lr_q=hp["lr_q"], lr_v=hp["lr_v"],
                              lr_actor=hp["lr_actor"], eps=hp["eps"], beta1=hp["beta1"], beta2=hp["beta2"])
        super().__init__("sac", cfg, self.P)

    def read(self):
        return {n: {k: v.cpu() for k, v in p.items()} for n, p in self.P.items()}

    def write(self, P):
        for n in P:
            for k in P[n]:
                self.P[n][k].copy_(P[n][k])

    def update(self, batch, eps):
        super().update(batch=batch_struct(S.cuda(batch) + (eps.float().cuda().contiguous(),)))


@pytest.mark.parametrize("case", S.SERIES_CASES, ids=S.series_id)
def test_fused_sac_adam_across_four_updates_matches_float64(case):
    """Four updates, a fresh tamed eps each, eps (Adam's) a power of two >= twice the first update's largest gradient element and
    re-asserted >= every element before each update, three different power-of-two learning rates, tau = 2^-4, margins re-planted
    in place before every update after the first: every tensor of Q, V, V_t and the actor within the series' bound (worst
    |got - want| / bound <= 1), every wrong variant rejected where sac_f64.SERIES_RULES says, V_t bit-identical under
    soft_update 0, the exact zeros bit for bit, and a new handle stepping as a fresh Adam and not as the carried one.

    Moments are observed only through the weights, and the margins are re-planted between updates: this is not a free-running
    trajectory."""
    shape, betas, mode, clamp_all = case
    res = A.run(S.series(shape, betas, mode, clamp_all, device="cuda"), Handle)
    print("worst/bound %s; smallest rejecting ratio %s" % ({n: "%.3g" % v for n, v in res["worst"].items()}, {k: "%.3g" % v for k, v in res["rejected"].items()}))
    assert max(res["worst"].values()) <= 1.0
