"""tri_accept (pt_kernels.hip; triangle.rs:297-303) is monotone in t_max: for fixed (t_scaled, det), a test accepted against a smaller
t_max is accepted against every larger one.  The pooled leaf round rests on it: the helper lanes apply the test with the owner's t_max
as the round starts, and since a ray's t_max never grows, what fails there fails against every t_max the owner's walk could have shown it.
Restated here in numpy float32, operation for operation (one IEEE multiply, eight compares, no fused operation)."""
import numpy as np

f32 = np.float32


def tri_accept(t_scaled, det, t_max):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        tmd = (t_max * det).astype(f32)
        rej_neg = (det < 0) & ((t_scaled >= 0) | (t_scaled < tmd))
        rej_pos = (det > 0) & ((t_scaled <= 0) | (t_scaled > tmd))
    return ~(rej_neg | rej_pos)


def _values(rng, n):
    """float32 values of every class: random bit patterns (all exponents, NaNs, denormals), ordinary magnitudes and the special values."""
    special = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, 3.4028235e38, -3.4028235e38,
                          1.0, -1.0], f32)
    pick = rng.integers(0, 4, n)
    raw = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(f32)
    normal = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(f32)
    den = (rng.integers(1, 2 ** 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(f32)
    return np.where(pick == 0, raw, np.where(pick == 1, normal, np.where(pick == 2, den, special[rng.integers(0, len(special), n)]))).astype(f32)


def test_accept_is_monotone_in_tmax():
    rng = np.random.default_rng(2024)
    n = 1000000
    t_scaled, det = _values(rng, n), _values(rng, n)
    assert np.isnan(t_scaled).any() and np.isnan(det).any() and (det < 0).any() and (det > 0).any() and (det == 0).any()
    assert (np.abs(t_scaled[np.isfinite(t_scaled)]) < 1.1754944e-38).any()
    # t_max is never negative or NaN (a ray's t_max starts non-negative and only takes accepted t values, which are positive)
    kinds = rng.integers(0, 4, (2, n))
    finite = np.abs(_values(rng, 2 * n))
    finite = np.where(np.isfinite(finite), finite, f32(1.0)).reshape(2, n)
    tiny = (rng.integers(1, 1 << 24, (2, n)).astype(np.uint32)).view(f32)                 # denormals and the smallest normals
    cand = np.where(kinds == 0, f32(0.0), np.where(kinds == 1, tiny, np.where(kinds == 2, finite, f32(np.inf)))).astype(f32)
    t0, t1 = np.maximum(cand[0], cand[1]), np.minimum(cand[0], cand[1])                   # t1 <= t0
    for k in range(4):
        assert (kinds[0] == k).any()
    a0, a1 = tri_accept(t_scaled, det, t0), tri_accept(t_scaled, det, t1)
    assert a1.any() and (~a1).any() and (a0 & ~a1).any()              # both outcomes occur, and t_max matters
    bad = a1 & ~a0
    assert not bad.any(), (t_scaled[bad][:5], det[bad][:5], t0[bad][:5], t1[bad][:5])

