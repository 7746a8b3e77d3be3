"""NumPy restatement of the packed actor-weight layout (include/crowdnav.h, cn_actor_pack_weights) and of what cn_actor_pop_pack
writes from an nn.Linear storage, for tests/test_actor_population_layout.py and tests/test_gpu_actor_population.py.

The header's formula, for a K-major matrix wt [K][256] with K a multiple of 32:
    packed[((((b*8 + w)*4 + q)*64 + lane)*4 + j] = wt[32 b + 4 (2 q + (j >> 1)) + (lane >> 4)][32 w + 2 (lane & 15) + (j & 1)]
cn_actor_pop_pack reads linear.weight W [256][K_in] (row-major, [out][in]) instead: the same element is W[c][k], and 0 where
k >= K_in (the zero rows that pad linear1 up to Dp = K_in rounded up to 32)."""
import numpy as np

H = 256


def padded(k_in):
    return (int(k_in) + 31) // 32 * 32


def packed_kc(K):
    """(k, c) of every index of a packed buffer of K rows: two int arrays [K * 256]."""
    idx = np.arange(K * H)
    j, lane, q, w, b = idx & 3, (idx >> 2) & 63, (idx >> 8) & 3, (idx >> 10) & 7, idx >> 13
    return 32 * b + 4 * (2 * q + (j >> 1)) + (lane >> 4), 32 * w + 2 * (lane & 15) + (j & 1)


def pack_kmajor(wt):
    """The header's formula applied to wt [K][256] (what cn_actor_pack_weights computes)."""
    wt = np.asarray(wt)
    K = wt.shape[0]
    assert wt.shape == (K, H) and K >= 32 and K % 32 == 0
    k, c = packed_kc(K)
    return wt[k, c]


def transposed_padded(W):
    """linear.weight [256][K_in] -> W^T zero-padded to [Dp][256]: the staging matrix the per-agent path builds."""
    W = np.asarray(W)
    wt = np.zeros((padded(W.shape[1]), H), dtype=W.dtype)
    wt[:W.shape[1]] = W.T
    return wt


def pack_from_linear(W):
    """What cn_actor_pop_pack writes for W [256][K_in]: one packed element per index, W[c][k] or 0 for k >= K_in."""
    W = np.asarray(W)
    K_in = W.shape[1]
    assert W.shape == (H, K_in)
    k, c = packed_kc(padded(K_in))
    flat = W.reshape(-1)
    return np.where(k < K_in, flat[(c * K_in + np.minimum(k, K_in - 1))], np.zeros((), dtype=W.dtype))


def pack_from_linear_no_zero_rows(W):
    """WRONG: the k < K_in test left out -- the padding rows read on into the next output's weights (wrapped at the end)."""
    W = np.asarray(W)
    K_in = W.shape[1]
    k, c = packed_kc(padded(K_in))
    return W.reshape(-1)[(c * K_in + k) % W.size]


def pack_from_linear_swapped(W):
    """WRONG: k and c exchanged -- the [out][in] storage indexed as if it were K-major [K_in][256]."""
    W = np.asarray(W)
    K_in = W.shape[1]
    k, c = packed_kc(padded(K_in))
    return np.where(k < K_in, W.reshape(-1)[(np.minimum(k, K_in - 1) * H + c) % W.size], np.zeros((), dtype=W.dtype))
