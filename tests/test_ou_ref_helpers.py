"""tests/ou_ref.py, the NumPy restatement of cn_ddpg_act's noise, against the reference's recorded Ornstein-Uhlenbeck process
(tests/golden/ddpg.npz: ou_u, ou_x, ou_reset_at, from the reference's own OUNoise) and the properties of the documented draw.  CPU only."""
import os

import numpy as np

import ou_ref

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ddpg.npz"))


def test_the_restated_update_reproduces_the_references_process_bit_for_bit():
    u, want, at = G["ou_u"], G["ou_x"], int(G["ou_reset_at"])
    assert u.shape == want.shape == (12, 2) and want.dtype == np.float64 and 0 < at < 12
    x = np.zeros((1, 2))
    for k in range(u.shape[0]):
        x = ou_ref.update(x, u[k:k + 1], reset=[k == at])
        assert np.array_equal(x[0], want[k]), k
    # the reset matters: without it the process leaves the recorded one at that call
    x = np.zeros((1, 2))
    for k in range(at + 1):
        x = ou_ref.update(x, u[k:k + 1])
    assert not np.array_equal(x[0], want[at])


def test_mix64_is_splitmix64s_finaliser():
    # splitmix64 seeded with 0: its first output is mix64(0) (Vigna's reference implementation)
    assert ou_ref.mix64(0) == 0xE220A8397B1DCDAF
    assert ou_ref.mix64(ou_ref.M64) < 1 << 64


def test_the_draw_is_a_multiple_of_2_to_the_minus_53_in_the_unit_interval():
    d = ou_ref.draws(seed=0x1234, counter=7, n=256)
    assert d.dtype == np.float64 and (d >= 0).all() and (d < 1).all()
    k = d * 2.0 ** 53
    assert np.array_equal(k, np.floor(k)) and (k < 2.0 ** 53).all()
    assert (np.floor(k) % 2 == 1).any()              # the lowest of the 53 bits is used


def test_the_draw_differs_between_rows_components_and_counters():
    a = ou_ref.draws(11, 3, 64)
    assert len(set(a.reshape(-1).tolist())) == 128                       # rows and components
    b = ou_ref.draws(11, 4, 64)
    assert not (a == b).any()                                            # counters
    assert not (a == ou_ref.draws(12, 3, 64)).any()                      # seeds
    # a row's draw depends on its key alone, not on how many rows the call has
    assert np.array_equal(ou_ref.draws(11, 3, 17), a[:17])


def test_the_draws_mean_over_4096_rows():
    """8 192 uniforms: the mean's standard error is sqrt(1 / 12 / 8192) = 0.0032; 0.02 is six of them."""
    d = ou_ref.draws(seed=0xD1B54A32D192ED03, counter=1, n=4096)
    assert abs(float(d.mean()) - 0.5) < 0.02
    assert abs(float(d[:, 0].mean()) - float(d[:, 1].mean())) < 0.04


def test_action_is_numpys_float32_add_of_a_float64_noise_then_the_clip():
    pi = np.array([[0.1, 1.5], [0.2, -1.9], [0.05, 0.3]], dtype=np.float32)
    x1 = np.array([[0.5, 0.9], [-0.4, -0.3], [0.01, 0.02]])
    want = np.clip((pi.astype(np.float64) + x1).astype(np.float32), [0.0, -2.0], [0.22, 2.0]).astype(np.float32)
    got = ou_ref.action(pi, x1)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert got[0, 0] == np.float32(0.22) and got[0, 1] == 2.0 and got[1, 0] == 0.0 and got[1, 1] == -2.0
