"""Motion blur without a GPU: the host's decompose() and motion_bounds against restatements, the ABI's new structures, and the proof
that the float64 truth of motion_ref.py decides the ray cases test_gpu_motion.py holds the device to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_cases as MC
import motion_ref as MR
from helpers import pkg, scenes

capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
U = 2.0 ** -24


def _m(t):
    return np.asarray(t[0], np.float32).reshape(4, 4)


def _shear():
    m = np.eye(4, dtype=np.float32)
    m[0, 1] = 0.3
    m[1, 2] = -0.2
    return m


def decompose_cases():
    T, S, R, mul = MC.T, MC.S, MC.rotate, MC.mul
    out = []
    for deg in (0.0, 1.0, 90.0, 179.0):
        for axis in ((0, 0, 1), (1, 2, 0.5), (-0.3, 1.0, 0.2)):
            out.append(("rigid %g about %s" % (deg, axis), _m(mul(T(0.5, -1.0, 2.0), R(deg, axis)))))
            out.append(("uniform scale %g about %s" % (deg, axis), _m(mul(T(-3.0, 0.25, 1.0), R(deg, axis), S(1.7, 1.7, 1.7)))))
            out.append(("non-uniform scale %g about %s" % (deg, axis), _m(mul(T(0.0, 4.0, -1.0), R(deg, axis), S(0.5, 2.0, 1.25)))))
    out.append(("mirror", _m(mul(T(1.0, 1.0, 1.0), R(40.0, (0, 1, 0)), S(-0.8, 0.8, 0.8)))))
    out.append(("mirror, two axes and a turn", _m(mul(R(75.0, (1, 1, 0)), S(-1.5, -0.6, 1.0)))))
    out.append(("shear", _shear()))
    out.append(("shear under a rotation", (_m(R(30.0, (0, 0, 1))) @ _shear()).astype(np.float32)))
    return out


CASES = decompose_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_decompose_against_its_float64_restatement(case):
    """pt_motion_decompose (float32) against decompose64 (the same algorithm, every operation widened).  T is copied: exact.  One round of
    the iteration re-projects through a normalised quaternion, so nothing accumulates over the rounds; the float32 result carries one
    round's roundings -- two 4 x 4 Gauss-Jordan inverses (gamma(16) each, Higham section 14.4), two 4 x 4 products (gamma(4)),
    Quaternion::from (a square root and a division on sums of three: gamma(6)), normalize (gamma(6)) and to_matrix (gamma(4)): gamma(56),
    rounded up to 64 u -- magnified by the conditioning of the two inversions involved: kappa = max |S| / min |S| for R (the scale is
    divided out of M and the quotient turned into a quaternion), once more for S = diag(R^-1 M), which is relative to max |S|.  kappa comes
    from the float64 decomposition.  The cases' scales lie in [0.5, 2]: kappa <= 4."""
    name, m = case
    T, R, S = capi.motion_decompose(m)
    T64, R64, S64 = MR.decompose64(m)
    kappa = np.abs(S64).max() / np.abs(S64).min()
    assert np.array_equal(T, T64.astype(np.float32))
    eR, eS = np.abs(R - R64).max(), np.abs(S - S64).max()
    bR, bS = 64 * U * kappa, 64 * U * kappa * np.abs(S64).max()
    print("%-44s kappa %.2f  |dR| %.2e of %.2e  |dS| %.2e of %.2e" % (name, kappa, eR, bR, eS, bS))
    assert eR <= bR and eS <= bS
    assert abs(float((R.astype(np.float64) ** 2).sum()) - 1.0) <= 8 * U and R[3] >= 0          # normalised, w >= 0 (Quaternion::new)


def test_decompose_quirks():
    """The scale is the diagonal of R^-1 M alone: a shear is dropped, and T R S does not give the matrix back.  A matrix without an
    inverse is refused."""
    m = _shear()
    T, R, S = capi.motion_decompose(m)
    back = np.eye(4)
    back[:3, :3] = MR.quat_matrix(R.astype(np.float64)) * S.astype(np.float64)
    assert np.abs(back[:3, :3] - m[:3, :3]).max() > 0.05          # the shear is gone ...
    Sfull = np.linalg.inv(MR.quat_matrix(R.astype(np.float64))) @ m[:3, :3].astype(np.float64)
    assert np.abs(np.diag(Sfull) - S).max() <= 64 * U and np.abs(Sfull - np.diag(np.diag(Sfull))).max() > 0.05      # ... because only the diagonal is kept
    with pytest.raises(capi.PtError):
        capi.motion_decompose(np.diag([1.0, 0.0, 1.0, 1.0]).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------- motion_bounds
def _interp32(rec32, t):
    """AnimatedTransform::interpolate's matrix in float32 numpy, operation for operation (the interpolating branch)."""
    T0, R0, S0, T1, R1, S1, t0, t1 = rec32
    one = f32(1)
    dt = f32(f32(t - t0) / f32(t1 - t0))
    tr = [f32(f32(f32(one - dt) * a) + f32(dt * b)) for a, b in zip(T0, T1)]
    sc = [f32(f32(f32(one - dt) * a) + f32(dt * b)) for a, b in zip(S0, S1)]
    c = f32(0)
    for a, b in zip(R0, R1):
        c = f32(c + f32(a * b))
    c = min(max(c, f32(0)), one)
    if c > f32(one - f32(2.0 ** -23)):
        q = list(R0)
    else:
        th = np.arccos(c, dtype=np.float32)
        s = f32(one / np.sin(th, dtype=np.float32))
        a_ = np.sin(f32(f32(one - dt) * th), dtype=np.float32)
        b_ = np.sin(f32(dt * th), dtype=np.float32)
        q = [f32(f32(f32(x * a_) + f32(y * b_)) * s) for x, y in zip(R0, R1)]
    x, y, z, w = q
    xx, yy, zz, xy, xz, yz, wx, wy, wz = f32(x * x), f32(y * y), f32(z * z), f32(x * y), f32(x * z), f32(y * z), f32(x * w), f32(y * w), f32(z * w)
    two = f32(2)
    r = [[f32(one - f32(two * f32(yy + zz))), f32(two * f32(xy - wz)), f32(two * f32(xz + wy))],
         [f32(two * f32(xy + wz)), f32(one - f32(two * f32(xx + zz))), f32(two * f32(yz - wx))],
         [f32(two * f32(xz - wy)), f32(two * f32(yz + wx)), f32(one - f32(two * f32(xx + yy)))]]
    m = np.eye(4, dtype=np.float32)
    for i in range(3):
        for j in range(3):
            m[i, j] = f32(r[i][j] * sc[j])
        m[i, 3] = tr[i]
    return m


def _bounds32(m, box):
    lo, hi = box[:3], box[3:]
    pts = []
    for c in range(8):
        p = [hi[0] if c & 4 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 1 else lo[2]]
        pts.append([f32(f32(f32(f32(m[i, 0] * p[0]) + f32(m[i, 1] * p[1])) + f32(m[i, 2] * p[2])) + m[i, 3]) for i in range(3)])
    pts = np.array(pts, np.float32)
    return np.concatenate([pts.min(0), pts.max(0)])


def _union(a, b):
    return np.concatenate([np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])])


def _motion_bounds32(start, end, times, box):
    """The three branches of AnimatedTransform::motion_bounds in float32 numpy, on the library's own decomposition."""
    d0, d1 = capi.motion_decompose(start), capi.motion_decompose(end)
    R1 = d1[1].copy()
    dot = f32(0)
    for a, b in zip(d0[1], R1):
        dot = f32(dot + f32(a * b))
    if dot < 0:
        R1 = -R1
        dot = f32(0)
        for a, b in zip(d0[1], R1):
            dot = f32(dot + f32(a * b))
    b0 = _bounds32(start, box)
    if np.array_equal(start, end):
        return b0, float(dot), "static"
    out = _union(b0, _bounds32(end, box))
    if not dot < f32(0.9995):
        return out, float(dot), "no rotation"
    t0, t1 = f32(times[0]), f32(times[1])
    rec = (d0[0], d0[1], d0[2], d1[0], R1, d1[2], t0, t1)
    for i in range(64):
        x = f32(f32(i) / f32(64))
        t = f32(f32(f32(f32(1) - x) * t0) + f32(x * t1))
        m = start if t <= t0 else (end if t1 <= t else _interp32(rec, t))
        out = _union(out, _bounds32(m, box))
    d = (out[3:] - out[:3]) * f32(0.1)
    return np.concatenate([out[:3] - d, out[3:] + d]).astype(np.float32), float(dot), "rotation"


BOX = np.array([-0.35, -0.5, -0.2, 0.4, 0.35, 0.6], np.float32)
BOUNDS_CASES = [
    ("equal ends", MC.T(1, 2, 3), MC.T(1, 2, 3)),
    ("translation", MC.T(-1, 0, 0.5), MC.T(2, 1, 0.5)),
    ("90 about a skew axis", MC.T(0, -1.3, 0.2), MC.mul(MC.T(0.5, -1, 0.5), MC.rotate(90.0, (1, 2, 0.5)))),
    ("120 and a non-uniform scale", MC.mul(MC.T(1.5, -1, 1), MC.S(1, 0.6, 1.4)), MC.mul(MC.T(1.5, -1, 1), MC.rotate(120.0, (0.3, 1, -0.2)), MC.S(1.3, 0.6, 1))),
    ("negative dot: 170 and -170 about z", MC.rotate(170.0, (0, 0, 1)), MC.rotate(-170.0, (0, 0, 1))),
    ("a mirror that turns", MC.mul(MC.rotate(10.0, (0, 1, 0)), MC.S(-0.8, 0.8, 0.8)), MC.mul(MC.T(0.3, 0.3, 0.4), MC.rotate(70.0, (0, 1, 0)), MC.S(-0.8, 0.8, 0.8))),
    ("a small turn: dot in [0.9995, 1)", MC.T(0, 0, 0), MC.rotate(2.0, (0, 0, 1))),
]


@pytest.mark.parametrize("case", BOUNDS_CASES, ids=[c[0] for c in BOUNDS_CASES])
def test_motion_bounds(case):
    """(1) pt_motion_bounds equals the float32 numpy restatement of the three branches.  The two sides share every operation but sinf and
    acosf (glibc's there, numpy's here; each within 1 ulp of the truth, so 2 ulp apart): through slerp's weights (|w| <= 1.5), the
    rotation's quadratic forms (factor 4), the scale (<= 2) and the corner sums (|corner| <= 1) that is below 32 ulp of the largest entry of
    the result, which is the allowance.  (2) With a real rotation (dot < 0.99) the bound contains the float64 image of the box's eight
    corners at 1 000 times.  A pair whose dot lies in [0.9995, 1) is held to the restatement only: the reference bounds it by its two ends
    while it slerps in between, and a point at radius r leaves that box by about r theta^2 / 8 -- a quirk of the reference, kept."""
    name, start, end = case
    s, e = _m(start), _m(end)
    times = [0.0, 1.0] if "skew" not in name else [2.0, 5.0]
    got = capi.motion_bounds(s, e, times, BOX)
    want, dot, branch = _motion_bounds32(s, e, times, BOX)
    allow = 32 * np.spacing(np.abs(want).max())
    print("%-40s dot %.6f  %-11s max |difference| %.2e of %.2e" % (name, dot, branch, np.abs(got - want).max(), allow))
    assert np.abs(got - want).max() <= allow
    assert branch == {"equal ends": "static", "translation": "no rotation", "a small turn: dot in [0.9995, 1)": "no rotation"}.get(name, "rotation")
    if "negative dot" in name:          # r[1] was negated: the short way round passes through angle 180, x = -r, not through angle 0
        assert got[0] < -0.5 and want[0] < -0.5
    if branch == "rotation" and dot < 0.99:
        inv = lambda m: np.linalg.inv(m.astype(np.float64)).astype(np.float32)
        rec = MR.Record(s, inv(s), e, inv(e), times)
        t = np.linspace(times[0], times[1], 1000).astype(np.float32)
        M = rec.instance_to_world(t)
        corners = np.array([[BOX[3 * ((c >> 2) & 1)], BOX[1 + 3 * ((c >> 1) & 1)], BOX[2 + 3 * (c & 1)], 1.0] for c in range(8)], np.float64)
        img = np.einsum("nij,cj->nci", M, corners)[:, :, :3]
        assert (img >= got[:3].astype(np.float64)).all() and (img <= got[3:].astype(np.float64)).all()


# ------------------------------------------------------------------------------------------------- the cases are decisive
def test_motion_ref_decides_the_ray_cases(oracle):
    """Condition of test_gpu_motion.py's ray test: motion_ref alone leaves out at most 3 % of its rays (geometry_ref's rules (a)-(d) under
    the enlarged bound).  The camera does not move in that scene, so the oracle's generator on the start-time scene makes the camera rays
    the device makes."""
    from test_texture_oracle import MAX_LEFT_OUT
    sd = MC.motion_instances()
    osc = oracle.scene(MC.motion_instances(at=0))
    rays = MC.make_rays(osc.generate_camera_rays, sd)
    osc.close()
    tr = MC.truth_of(sd, rays)
    left = float((tr["rule"] != 0).mean())
    by = np.bincount(tr["rule"], minlength=5)
    time = rays[4]
    print("motion_instances: left out %.2f %% (a %d, b %d, c %d, d %d of %d), %d hits" % (100 * left, by[1], by[2], by[3], by[4], len(time), (tr["kind"] > 0).sum()))
    assert left <= MAX_LEFT_OUT == 0.03
    assert (tr["kind"] > 0).sum() >= 1000
    for prim in (0, 1, 2, 5, 6, 7, 8, 9):          # every instance is met by decisive rays
        assert ((tr["prim"] == prim) & (tr["rule"] == 0)).sum() >= 30, prim
    assert ((time > 0) & (time < 1) & np.isin(tr["prim"], [0, 1, 2, 7, 8, 9]) & (tr["rule"] == 0)).sum() > 300
    # and the truth moves: the same rays at time 0 meet something else
    tr0 = MR.closest_hits(sd, rays[0], rays[1], rays[2], np.zeros(len(time), np.float32))
    assert (tr0["prim"] != tr["prim"]).mean() > 0.02


@pytest.mark.parametrize("name", ["aov", "shadow", "ao"])
def test_motion_ref_decides_the_rendered_cases(oracle, name):
    """The same condition for the rendered cases of test_gpu_motion_integrators.py: at most 3 % left out by the truth alone.  Their
    cameras do not move, so the oracle's scene at the start transforms (under `path`: the oracle is asked for camera samples only) gives
    the device's camera rays and sampler values."""
    import motion_integrator_cases as IC
    static = IC.near_scene("path", moving=False) if name == "aov" else IC.shadow_scene(moving=False)
    osc = oracle.scene(static)
    case = {"aov": IC.aov_case, "shadow": IC.shadow_case, "ao": IC.ao_case}[name](osc)
    osc.close()
    print("%s: left out %.2f %%" % (name, 100 * case["left"]))
    assert case["left"] <= IC.MAX_LEFT_OUT == 0.03
    tm = case["time"]
    assert ((tm > 0) & (tm < 1)).mean() > 0.95
    if name == "aov":
        tr = case["truth"]
        assert ((tr["rule"] == 0) & np.isin(tr["prim"], IC.NEAR_MOVING_PRIMS)).sum() > 2000
    elif name == "shadow":
        dec, occ = case["decisive"], case["occluded"]
        assert (dec & occ).sum() > 200 and (dec & ~occ).sum() > 200
    else:
        hist = np.bincount(case["n_occluded"][case["decisive"]], minlength=5)
        assert hist[1:].sum() > 200 and hist[0] > 200


def test_truth_at_the_ends_is_the_static_truth():
    """At t <= t0 and t1 <= t the truth is geometry_ref's own on the static scenes built from the start and the end transforms."""
    import geometry_ref as G
    sd = MC.motion_instances()
    rng = np.random.default_rng(2)
    n = 2000
    o = np.tile(np.array([0, 0, -6.5], np.float32), (n, 1))
    d = rng.standard_normal((n, 3)).astype(np.float32) * 0.25
    d[:, 2] = 1.0
    tmax = np.full(n, np.inf, np.float32)
    for at, tm in ((0, -0.05), (0, 0.0), (1, 1.0), (1, 1.3)):
        a = MR.closest_hits(sd, o, d, tmax, np.full(n, tm, np.float32))
        b = G.closest_hits(G.Scene(MC.motion_instances(at=at)), o, d, tmax)
        assert (a["kind"] > 0).sum() > 300
        for k in ("kind", "prim", "rule", "occluded"):
            assert np.array_equal(a[k], b[k]), (at, tm, k)
        for k in ("t", "bound"):          # (one matrix per ray is summed in another order than one matrix for all: float64 roundings)
            assert np.allclose(a[k], b[k], rtol=1e-12, atol=0.0), (at, tm, k)


# --------------------------------------------------------------------------------------------------------- structures, ABI
def test_structures_match_the_header_and_the_abi_number_stays(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbrtgpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(pt_motion), '
                   'sizeof(pt_motion_instance), offsetof(pt_motion, camera_to_world_end), offsetof(pt_motion, instances), '
                   'offsetof(pt_motion_instance, world_to_instance_end), PT_KERNELS_MOTION, PT_ABI_VERSION);return 0;}\n')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    mine = [C.sizeof(capi.pt_motion), C.sizeof(capi.pt_motion_instance), capi.pt_motion.camera_to_world_end.offset, capi.pt_motion.instances.offset,
            capi.pt_motion_instance.world_to_instance_end.offset, capi.PT_KERNELS_MOTION, 9]
    assert got == mine
    lib = capi.load_library()
    assert lib.pt_abi_version() == 9
    for s in ("pt_scene_set_motion", "pt_trace_closest_time", "pt_trace_any_time", "pt_trace_wavefront_time", "pt_generate_camera_rays_time",
              "pt_motion_decompose", "pt_motion_bounds"):
        assert hasattr(lib, s), s


def test_scene_builder_yields_the_implicit_object():
    """animated_shape_begin / _end: the shapes under the identity as one object with one moving instance at that place of the world list,
    and no area light (scene_context.rs:1233-1293)."""
    b = scenes.SceneBuilder()
    b.transform_times(2.0, 5.0)
    b.area_light_source_diffuse(L=(5, 5, 5))
    scenes._quad(b, (1, 0, 0), (0, 0, 0), (0, 0, 1), (1, 0, 1))
    b.animated_shape_begin(MC.T(0, 1, 0), MC.T(0, 2, 0))
    b.shape_trianglemesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [0, 1, 2])
    b.animated_shape_end()
    scenes._quad(b, (1, 3, 0), (0, 3, 0), (0, 3, 1), (1, 3, 1))
    sd = b.build()
    d = sd.desc
    assert d.n_instances == 1 and sd.motion.n_instances == 1 and list(sd.motion.transform_times) == [2.0, 5.0]
    meshes = [sd.buffers["meshes"][i] for i in range(d.n_meshes)]
    assert [m.object for m in meshes] == [0, 1, 0] and [m.area_light for m in meshes] == [0, -1, 0]
    assert sd.buffers["instances"][0].before_triangle == 3 and sd.motion.instances[0].instance_to_world_end[7] == 2.0
    P = np.asarray(sd.buffers["P"]).reshape(-1, 3)
    assert np.array_equal(P[4:7], np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32))          # built under the identity
