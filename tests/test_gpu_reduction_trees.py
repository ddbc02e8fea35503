"""-m gpu test that pins the two workgroup summation trees of csrc/wg_dev.h to NumPy replays, bit for bit.

Tree A (LDS tree) through the means of gpemu_marginal_moments_dev, tree B (wave tree) through the means of
gpemu_weighted_moments_dev with all log-weights 0.  Both mean passes are pure additions (x - 0.0, 1.0 * x) followed by
one correctly rounded division, so the replay must give the device's bits exactly.  Only the variance passes (products,
possibly contracted to FMA) are left unpinned.  The tree B case relies on exp(0.0) == 1.0 on the device.

The inputs are normal * 10**uniform(-3, 3), so that every level of a tree rounds.  On the host the test also checks that
the pin is not vacuous: for the chosen seeds the replay with the OTHER tree, and np.sum, each differ from the expected
bits in at least one column."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MOM_ROWS = 1024      # rows_dev.h
LOO_SUM = 4096       # the chunk of k_loo.hip's sums


def tree_a(v):
    """red[t] = v[t]; for off = n/2 .. 1: red[t] += red[t + off], t < off; red[0].  v: (n, columns)"""
    red = np.array(v, dtype=np.float64)
    off = red.shape[0] // 2
    while off > 0:
        red[:off] = red[:off] + red[off:2 * off]
        off //= 2
    return red[0]


def tree_b(v):
    """the xor butterfly 32 .. 1 within each wave of 64, then the waves left to right from ws[0].  v: (64 waves, columns)"""
    v = np.array(v, dtype=np.float64).reshape(-1, 64, v.shape[-1])
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    out = v[0, 0]
    for w in range(1, v.shape[0]):
        out = out + v[w, 0]
    return out


def strided(x, n_threads, per_thread):
    """thread t adds the rows t, t + n_threads, ... of x (at most per_thread, absent rows: nothing) from 0.0, in order"""
    pad = np.zeros((n_threads * per_thread, x.shape[1]))
    pad[:x.shape[0]] = x
    live = (np.arange(n_threads * per_thread) < x.shape[0]).reshape(per_thread, n_threads)
    acc = np.zeros((n_threads, x.shape[1]))
    for q, rows in enumerate(pad.reshape(per_thread, n_threads, -1)):
        acc = np.where(live[q][:, None], acc + rows, acc)
    return acc


def replay_marginal_mean(x, tree):
    """launch_moments' mean: per block of MOM_ROWS thread t adds rows t, t + 256, ..., the tree over 256; thread t adds
    the block partials t, t + 256, ..., the tree again; / S"""
    S = x.shape[0]
    part = np.array([tree(strided(x[r0:r0 + MOM_ROWS], 256, MOM_ROWS // 256)) for r0 in range(0, S, MOM_ROWS)])
    return tree(strided(part, 256, (part.shape[0] + 255) // 256)) / float(S)


def replay_weighted_mean(x, tree):
    """wm_partial_kernel / wm_finish_kernel with w = 1: per chunk of LOO_SUM every lane adds its 16 elements in index
    order, the tree over 256; the chunks in order from 0.0; / S"""
    S = x.shape[0]
    total = np.zeros(x.shape[1])
    for c0 in range(0, S, LOO_SUM):
        total = total + tree(strided(x[c0:c0 + LOO_SUM], 256, LOO_SUM // 256))
    return total / float(S)


def inputs(seed, S, d):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(S, d)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(S, d))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("S", [1500, 255])     # two blocks, the second ragged (476 rows); a thread with nothing to add
def test_tree_a_marginal_means_equal_the_replay(S):
    import torch
    from gpemu import marginals as M
    d = 3
    x = inputs(20260 + S, S, d)
    want = replay_marginal_mean(x, tree_a)
    other, plain = replay_marginal_mean(x, tree_b), np.sum(x, axis=0) / float(S)
    assert np.any(bits(other) != bits(want)), "the seed does not tell tree A from tree B"
    assert np.any(bits(plain) != bits(want)), "the seed does not tell tree A from np.sum"
    dx = torch.from_numpy(x).cuda()
    mean, _ = M._moments_dev(0, dx.data_ptr(), S, d)
    print(f"S={S}: device {mean.tolist()} replay {want.tolist()}")
    assert np.array_equal(bits(mean), bits(want))


def test_tree_b_weighted_means_equal_the_replay():
    import torch
    from gpemu import loo
    S, d = 5000, 2                                 # chunks of 4096 + 904
    x = inputs(20262, S, d)
    want = replay_weighted_mean(x, tree_b)
    other, plain = replay_weighted_mean(x, tree_a), np.sum(x, axis=0) / float(S)
    assert np.any(bits(other) != bits(want)), "the seed does not tell tree B from tree A"
    assert np.any(bits(plain) != bits(want)), "the seed does not tell tree B from np.sum"
    dx = torch.from_numpy(x).cuda()
    lw = torch.zeros((1, S), dtype=torch.float64, device="cuda")
    mean, _ = loo.weighted_moments_dev(0, dx.data_ptr(), 1, S, S, d, lw)
    print(f"device {mean[0].tolist()} replay {want.tolist()}")
    assert np.array_equal(bits(mean[0]), bits(want))
