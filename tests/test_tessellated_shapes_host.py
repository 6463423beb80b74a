"""Shapes "loopsubdiv", "nurbs" and "heightfield" on the host (no device needed).

The library's tessellators (pth_tessellate_*) and the front end's meshes are held bit for bit to tests/tessellate_ref.py, an
independent float32 restatement of shapes/loopsubdiv.rs, shapes/nurbs.rs and shapes/heightfield.rs: positions, normals (NaN
where the reference has NaN), uv, indices and their order.  Then the parameters, scoping, errors and the SceneBuilder methods."""
import numpy as np
import pytest

import tess_inputs as ti
import tessellate_ref as ref
from helpers import bits, pkg, scenes

capi = pkg.capi
HEAD = 'Sampler "sobol"\nWorldBegin\n'
LIGHT = 'AttributeBegin\nAreaLightSource "diffuse"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 9 1 0 9 0 1 9]\nAttributeEnd\n'


def same(a, b):
    """Bit-identical arrays (None = absent on both sides)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)                     # a NaN is a NaN, whatever its sign bit after a transform
    return np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def assert_mesh(got, want):
    for k in ("P", "N", "uv"):
        assert same(got[k], want[k]), k
    assert np.array_equal(got["indices"].astype(np.int64), want["indices"].astype(np.int64))


def parse(body, work_dir=None):
    return capi.ParsedScene(text=HEAD + body + "WorldEnd\n", work_dir=work_dir)


def desc_mesh(ps, mesh_id):
    """Vertices and triangles of one pt_mesh of a parsed scene: (P, N, UV, indices local to the mesh, pt_mesh)."""
    d = ps.desc
    nv, nt = d.n_vertices, d.n_triangles
    idx = np.ctypeslib.as_array(d.indices, (nt * 3,)).reshape(-1, 3).astype(np.int64)
    tm = np.ctypeslib.as_array(d.tri_mesh, (nt,))
    tri = idx[tm == mesh_id]
    arr = lambda p, w: np.ctypeslib.as_array(p, (nv * w,)).reshape(-1, w) if p else None
    P, N, UV = arr(d.P, 3), arr(d.N, 3), arr(d.UV, 2)
    m = d.meshes[mesh_id]
    return P, N, UV, tri, m


def expect_in_scene(t):
    """What emit_mesh makes of object-space arrays under the identity CTM: P through transform_point, the area filter."""
    P = scenes._transform_points(np.eye(4, dtype=np.float32).reshape(-1), t["P"])
    keep = scenes._tri_areas(P, t["indices"].astype(np.int64)) > np.float32(1e-16)
    return P, t["indices"][keep].astype(np.int64)


def check_parsed(body, t, mesh_id=1, base=3):
    """The scene (LIGHT first: mesh 0, vertices 0..2) holds `t` as mesh `mesh_id` starting at vertex `base`."""
    ps = parse(LIGHT + body)
    P, N, UV, tri, m = desc_mesh(ps, mesh_id)
    wantP, wantI = expect_in_scene(t)
    n = len(t["P"])
    assert ps.desc.n_vertices == base + n
    assert same(P[base:base + n], wantP)
    assert np.array_equal(tri - base, wantI)
    if t["N"] is not None:
        assert m.flags & capi.PT_MESH_HAS_N and same(N[base:base + n], scenes._transform_normals(np.eye(4, dtype=np.float32).reshape(-1), t["N"]))
    else:
        assert not m.flags & capi.PT_MESH_HAS_N
    if t["uv"] is not None:
        assert m.flags & capi.PT_MESH_HAS_UV and same(UV[base:base + n], t["uv"])
    else:
        assert not m.flags & capi.PT_MESH_HAS_UV
    return ps, m


# ---------------------------------------------------------------- loopsubdiv: exact
LOOP_MESHES = {
    "tetrahedron": ti.tetrahedron,
    "icosahedron": ti.icosahedron,
    "grid": lambda: ti.grid(3, 3, flip=lambda x, y: (x + 2 * y) % 3 == 0),
    "grid_corners": lambda: ti.grid(2, 1, flip=lambda x, y: x == 1),
    "fan_boundary_7": lambda: ti.fan(8),
    "fan_boundary_2": lambda: ti.fan(2),
    "valence_3_to_12": ti.valence_mesh,
}


# levels 0 ... 4; the valence mesh stops at 3 (level 4 is 38 400 faces through the pure-Python restatement)
@pytest.mark.parametrize("name,levels", [(n, l) for n in LOOP_MESHES for l in range(5) if not (n == "valence_3_to_12" and l > 3)])
def test_loopsubdiv_matches_restatement(name, levels):
    P, I = LOOP_MESHES[name]()
    want = ref.loopsubdiv(I, P, levels)
    got = capi.tessellate_loopsubdiv(I, P, levels)
    assert_mesh(got, want)
    assert got["uv"] is None and len(got["indices"]) == (len(I) // 3) * 4 ** levels


def test_loopsubdiv_boundary_valences_are_exercised():
    """The open grids and fans reach every boundary branch of the limit tangent (valence 2, 3, 4 and other)."""
    seen = set()
    for name in ("grid", "grid_corners", "fan_boundary_7", "fan_boundary_2"):
        P, I = LOOP_MESHES[name]()
        F = I.reshape(-1, 3)
        E = set()
        for f in F:
            for k in range(3):
                E.add((f[k], f[(k + 1) % 3]))
        val = np.bincount(F.reshape(-1), minlength=len(P))
        for v in range(len(P)):
            on_boundary = any((a == v or b == v) and (b, a) not in E for (a, b) in E)
            if on_boundary:
                seen.add(min(int(val[v]) + 1, 5))
    assert seen >= {2, 3, 4, 5}


def test_loopsubdiv_random_manifolds():
    rng = np.random.default_rng(20261016)
    for case in range(300):
        P, I = ti.random_manifold(rng)
        levels = int(rng.integers(0, 3))
        want = ref.loopsubdiv(I, P, levels)
        got = capi.tessellate_loopsubdiv(I, P, levels)
        try:
            assert_mesh(got, want)
        except AssertionError as e:
            raise AssertionError("case %d (levels %d): %s" % (case, levels, e))


# ---------------------------------------------------------------- nurbs: exact
NURBS_CASES = {
    "bilinear": dict(nu=2, nv=2, uorder=2, vorder=2, uknots=[0, 0, 1, 1], vknots=[0, 0, 1, 1], P=[0, 0, 0, 1, 0, .2, 0, 1, .1, 1, 1, -.3], diceu=4, dicev=3),
    "bicubic_bezier": dict(nu=4, nv=4, uorder=4, vorder=4, uknots=[0, 0, 0, 0, 1, 1, 1, 1], vknots=[0, 0, 0, 0, 1, 1, 1, 1],
                           P=np.random.default_rng(1).normal(0, 1, 48), diceu=9, dicev=7),
    "uniform_open": dict(nu=5, nv=4, uorder=3, vorder=2, uknots=[0, 1, 2, 3, 4, 5, 6, 7], vknots=[0, 1, 2, 3, 4, 5],
                         P=np.random.default_rng(2).normal(0, 1, 60)),
    "nonuniform_rational": dict(nu=6, nv=5, uorder=4, vorder=3, uknots=[0, 0, 0, 0, .3, .35, 1, 1, 1, 1], vknots=[0, 0, 0, .2, .7, 1, 1, 1],
                                Pw=np.concatenate([np.random.default_rng(3).normal(0, 1, (30, 3)) * 0.7, np.random.default_rng(4).uniform(.4, 2, (30, 1))], 1),
                                diceu=11, dicev=6),
    "range_outside_knots": dict(nu=4, nv=3, uorder=3, vorder=3, uknots=[0, 0, 0, .5, 1, 1, 1], vknots=[0, 0, 0, 1, 1, 1],
                                P=np.random.default_rng(5).normal(0, 1, 36), u0=-2.0, u1=0.75, v0=0.25, v1=7.0, diceu=5, dicev=5),
    "dice_below_two": dict(nu=3, nv=3, uorder=3, vorder=3, uknots=[0, 0, 0, 1, 1, 1], vknots=[0, 0, 0, 1, 1, 1],
                           P=np.random.default_rng(6).normal(0, 1, 27), diceu=0, dicev=-4),
    "sphere_with_poles": dict(ti.nurbs_sphere(), diceu=13, dicev=9),
    "sphere_default_dice": ti.nurbs_sphere(),
}


@pytest.mark.parametrize("name", list(NURBS_CASES))
def test_nurbs_matches_restatement(name):
    kw = NURBS_CASES[name]
    want = ref.nurbs(**kw)
    got = capi.tessellate_nurbs(**kw)
    assert_mesh(got, want)
    if name.startswith("sphere"):
        assert np.isnan(got["N"]).any(axis=1).sum() > 0      # the poles: the reference's normals are NaN there, and so are these


def test_nurbs_random_patches():
    """Random patches; where the restatement meets one of the reference's asserts the library refuses the patch."""
    rng = np.random.default_rng(7)
    refused = 0
    for case in range(200):
        kw = ti.random_nurbs(rng)
        try:
            want = ref.nurbs(**kw)
        except (AssertionError, IndexError):
            with pytest.raises(capi.PtError, match="nurbs"):
                capi.tessellate_nurbs(**kw)
            refused += 1
            continue
        try:
            assert_mesh(capi.tessellate_nurbs(**kw), want)
        except AssertionError as e:
            raise AssertionError("case %d %r: %s" % (case, kw, e))
    assert refused < 100


# ---------------------------------------------------------------- heightfield: exact
@pytest.mark.parametrize("nu,nv,z", [(2, 2, [0, 0, 0, 0]), (2, 2, [1, -2, 0.5, -0.0]), (3, 5, None), (7, 2, None), (1, 4, [1, 2, 3, 4])])
def test_heightfield_matches_restatement(nu, nv, z):
    if z is None:
        z = np.random.default_rng(nu * 10 + nv).normal(0, 2, nu * nv).astype(np.float32)
        z[::3] = 0.0
    want = ref.heightfield(nu, nv, z)
    got = capi.tessellate_heightfield(nu, nv, z)
    assert_mesh(got, want)


# ---------------------------------------------------------------- the front end: same arrays in the scene
def test_parsed_loopsubdiv_equals_restatement():
    P, I = ti.icosahedron()
    ps, m = check_parsed(ti.loopsubdiv_text(P, I, 2), ref.loopsubdiv(I, P, 2))
    assert m.flags & capi.PT_MESH_TWO_SIDED
    P, I = LOOP_MESHES["grid"]()
    check_parsed(ti.loopsubdiv_text(P, I), ref.loopsubdiv(I, P, 3))            # default levels 3


def test_parsed_nurbs_and_heightfield_equal_restatement():
    for kw in (NURBS_CASES["nonuniform_rational"], NURBS_CASES["sphere_with_poles"], NURBS_CASES["range_outside_knots"]):
        check_parsed(ti.nurbs_text(kw), ref.nurbs(**kw))
    z = np.random.default_rng(9).normal(0, 1, 12).astype(np.float32)
    check_parsed(ti.heightfield_text(4, 3, z), ref.heightfield(4, 3, z))


def test_shapes_were_refused_before():
    """All three names reach the tessellators (the front end used to stop at them)."""
    P, I = ti.tetrahedron()
    for body in (ti.loopsubdiv_text(P, I, 1), ti.nurbs_text(NURBS_CASES["bilinear"]), ti.heightfield_text(2, 2, [0, 1, 2, 3])):
        ps = parse(body)
        assert ps.desc.n_triangles > 0 and ps.desc.n_meshes == 1


# ---------------------------------------------------------------- parameters
def test_levels_over_nlevels():
    P, I = ti.tetrahedron()
    def n(extra):
        ps = parse('Shape "loopsubdiv" "integer indices" [%s] "point P" [%s]%s\n' % (ti._arr(I, str), ti._arr(P), extra))
        return ps.desc.n_triangles
    assert n("") == 4 * 4 ** 3
    assert n(' "integer nlevels" [1]') == 16
    assert n(' "integer levels" [2]') == 64
    assert n(' "integer levels" [0] "integer nlevels" [2]') == 4
    assert n(' "integer nlevels" [2] "integer levels" [1] "string scheme" "butterfly"') == 16


def test_twosided_rules():
    P, I = ti.tetrahedron()
    def flag(body):
        ps = parse(body)                                    # (the desc lives as long as the parsed scene)
        return ps.desc.meshes[0].flags & capi.PT_MESH_TWO_SIDED
    assert flag(ti.loopsubdiv_text(P, I, 1))
    assert not flag(ti.loopsubdiv_text(P, I, 1, ' "bool twosided" "false"'))
    assert flag(ti.nurbs_text(NURBS_CASES["bilinear"], ' "bool twosided" "false"'))          # create_triangle_mesh gets an empty ParamSet
    assert flag(ti.heightfield_text(2, 2, [0, 0, 0, 1], ' "bool twosided" "false"'))


def test_no_uv_fill_and_no_alpha_masks():
    P, I = ti.tetrahedron()
    ps = parse('Texture "ck" "float" "checkerboard"\n' + ti.loopsubdiv_text(P, I, 1, ' "float alpha" [0] "texture shadowalpha" "ck"')
               + ti.nurbs_text(NURBS_CASES["bilinear"], ' "float alpha" [0]') + ti.heightfield_text(2, 2, [0, 0, 0, 1], ' "float shadowalpha" [0]')
               + 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0] "float alpha" [0]\n')
    assert [m.mesh for m in ps.alpha_masks] == [3]                 # only the trianglemesh
    d = ps.desc
    assert not d.meshes[0].flags & capi.PT_MESH_HAS_UV            # loopsubdiv: no uv, and no (0,0) (1,0) (1,1) fill
    assert d.meshes[1].flags & capi.PT_MESH_HAS_UV and d.meshes[2].flags & capi.PT_MESH_HAS_UV
    assert not d.meshes[2].flags & capi.PT_MESH_HAS_N


def test_material_from_shape_parameters():
    P, I = ti.tetrahedron()
    """Shape parameters fill what the material leaves unset (material first, then shape: texture_params.rs:36-54)."""
    ps = parse('Material "matte"\n' + ti.loopsubdiv_text(P, I, 1, ' "rgb Kd" [0.9 0.1 0.1]')
               + ti.nurbs_text(NURBS_CASES["bilinear"], ' "rgb Kd" [0.1 0.9 0.1]') + ti.heightfield_text(2, 2, [0, 0, 0, 1]))
    d = ps.desc
    kd = [tuple(np.float32(d.materials[d.meshes[i].material].kd)) for i in range(3)]
    assert kd == [tuple(np.float32([0.9, 0.1, 0.1])), tuple(np.float32([0.1, 0.9, 0.1])), tuple(np.float32([0.5, 0.5, 0.5]))]


def test_area_light_per_triangle():
    P, I = ti.tetrahedron()
    ps = parse('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1]\n' + ti.loopsubdiv_text(P, I, 1) + 'AttributeEnd\n')
    d = ps.desc
    assert d.n_area_lights == 1 and d.meshes[0].area_light == 0 and d.n_triangles == 16


# ---------------------------------------------------------------- scoping and transforms
def test_object_instancing_reverse_orientation_and_handedness():
    P, I = ti.icosahedron()
    t = ref.loopsubdiv(I, P, 1)
    ps = parse('ObjectBegin "blob"\n' + ti.loopsubdiv_text(P, I, 1) + ti.heightfield_text(2, 3, [0, 1, 2, 3, 4, 5]) + 'ObjectEnd\n'
               'AttributeBegin\nTranslate 3 0 0\nObjectInstance "blob"\nAttributeEnd\nAttributeBegin\nScale 1 1 -1\nObjectInstance "blob"\nAttributeEnd\n'
               'AttributeBegin\nReverseOrientation\nScale -1 1 1\n' + ti.loopsubdiv_text(P, I, 1, ' "bool twosided" "false"') + 'AttributeEnd\n')
    d = ps.desc
    assert d.n_meshes == 3 and d.n_instances == 2
    assert d.meshes[0].object == 1 and d.meshes[1].object == 1 and d.meshes[2].object == 0
    f = d.meshes[2].flags
    assert f & capi.PT_MESH_REVERSE_ORIENTATION and f & capi.PT_MESH_SWAPS_HANDEDNESS and not f & capi.PT_MESH_TWO_SIDED
    nv = len(t["P"])
    base = nv + 6
    P2 = np.ctypeslib.as_array(d.P, (d.n_vertices * 3,)).reshape(-1, 3)[base:base + nv]
    N2 = np.ctypeslib.as_array(d.N, (d.n_vertices * 3,)).reshape(-1, 3)[base:base + nv]
    m, minv = scenes.transform_scale(-1, 1, 1)
    assert same(P2, scenes._transform_points(m, t["P"]))
    assert same(N2, scenes._transform_normals(minv, t["N"]))


# ---------------------------------------------------------------- errors
TET_P, TET_I = ti.tetrahedron()
ERRORS = [
    ('Shape "loopsubdiv" "point P" [0 0 0 1 0 0 0 1 0]', 'Vertex indices "indices" not provided for LoopSubdiv shape.'),
    ('Shape "loopsubdiv" "integer indices" [0 1 2]', 'Vertex positions "P" not provided for LoopSubdiv shape.'),
    ('Shape "loopsubdiv" "integer levels" [-1] "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]', "negative"),
    ('Shape "loopsubdiv" "integer indices" [0 1 3] "point P" [0 0 0 1 0 0 0 1 0]', "out of range"),
    ('Shape "loopsubdiv" "integer indices" [0 1 2 1 0 3 0 1 4] "point P" [0 0 0 1 0 0 0 1 0 0 -1 0 0 0 1]', "more than two faces"),
    ('Shape "loopsubdiv" "integer indices" [0 1 2 0 1 3] "point P" [0 0 0 1 0 0 0 1 0 0 -1 0]', "wound inconsistently"),
    ('Shape "loopsubdiv" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0 5 5 5]', "belongs to no face"),
    ('Shape "loopsubdiv" "integer indices" [0 1 1] "point P" [0 0 0 1 0 0 0 1 0]', "repeats a vertex"),
    ('Shape "nurbs" "integer uorder" [2]', 'Must provide number of control points "nu" with NURBS shape.'),
    ('Shape "nurbs" "integer nu" [2]', 'Must provide u order "uorder" with NURBS shape.'),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2]', 'Must provide u knot vector "uknots" with NURBS shape.'),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1]',
     "Number of knots in u knot vector 3 doesn't match sum of number of u control points 2 and u order 2."),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1]', 'Must provide number of control points "nv" with NURBS shape.'),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1] "integer nv" [2]', 'Must provide v order "vorder" with NURBS shape.'),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1] "integer nv" [2] "integer vorder" [2]',
     'Must provide v knot vector "vknots" with NURBS shape.'),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 1 1 1 1]',
     "Number of knots in v knot vector 5 doesn't match sum of number of v control points 2 and v order 2."),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1]',
     'Must provide control points via "P" or "Pw" parameter to NURBS shape.'),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] "point P" [0 0 0 1]',
     "Number of control points must be multiple of 3 or 4."),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] "point P" [0 0 0 1 0 0 0 1 0]',
     "Number of control points 3 doesn't match nu * nv = 2 * 2 = 4."),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] "point4 Pw" [0 0 0 1 1 0 0 1 0 1 0 1]',
     "Number of control points 3 doesn't match nu * nv = 2 * 2 = 4."),
    ('Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 1 0.5 0] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] "point P" [0 0 0 1 0 0 0 1 0 1 1 0]',
     "empty parameter range"),
    ('Shape "nurbs" "integer nu" [3] "integer uorder" [3] "float uknots" [0 0 1 1 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] "point P" [%s]'
     % " ".join(["0 0 0"] * 6), "cannot be evaluated"),
    ('Shape "nurbs" "integer nu" [1] "integer uorder" [1] "float uknots" [0 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] "point P" [0 0 0 1 0 0]',
     "orders outside"),
    ('Shape "heightfield" "integer nu" [2] "float Pz" [0 0 0 0]', 'Must provide "nu" and "nv" parameters to heightfield shape.'),
    ('Shape "heightfield" "integer nu" [2] "integer nv" [2]', "No vertex positions provided for heightfield shape."),
    ('Shape "heightfield" "integer nu" [2] "integer nv" [2] "float Pz" [0 0 0]', "Number of \"Pz\" values doesn't match resolution."),
    ('Shape "heightfield" "integer nu" [0] "integer nv" [2] "float Pz" []', "must be positive"),
]


@pytest.mark.parametrize("body,needle", ERRORS)
def test_errors_name_the_shape(body, needle):
    shape = body.split('"')[1]
    with pytest.raises(capi.PtError) as e:
        parse(body + "\n")
    msg = str(e.value)
    assert needle in msg and ('Shape "%s"' % shape) in msg, msg


def test_entry_points_refuse_with_the_shape_name():
    with pytest.raises(capi.PtError, match="loopsubdiv: .*more than two faces"):
        capi.tessellate_loopsubdiv([0, 1, 2, 1, 0, 3, 0, 1, 4], np.zeros(15), 1)
    with pytest.raises(capi.PtError, match="loopsubdiv: .*not provided"):
        capi.tessellate_loopsubdiv(None, np.zeros(9), 1)
    with pytest.raises(capi.PtError, match="nurbs: Must provide control points"):
        capi.tessellate_nurbs(2, 2, 2, 2, [0, 0, 1, 1], [0, 0, 1, 1])
    with pytest.raises(capi.PtError, match="heightfield: No vertex positions"):
        capi.tessellate_heightfield(2, 2, None)


def test_non_manifold_inputs_do_not_crash():
    """Edges shared by three or four faces, mixed winding, bow-ties: refused or tessellated, never a crash or a hang."""
    rng = np.random.default_rng(11)
    for _ in range(200):
        nv = int(rng.integers(3, 9))
        I = rng.integers(0, nv, 3 * int(rng.integers(1, 10)))
        P = rng.normal(0, 1, 3 * nv)
        levels = int(rng.integers(0, 3))
        try:
            t = capi.tessellate_loopsubdiv(I, P, levels)
        except capi.PtError as e:
            assert "loopsubdiv" in str(e)
            continue
        assert_mesh(t, ref.loopsubdiv(I, P, levels))           # accepted: a manifold the restatement handles too


# ---------------------------------------------------------------- SceneBuilder
def test_scene_builder_equals_parsed_scene():
    P, I = ti.icosahedron()
    kw = NURBS_CASES["nonuniform_rational"]
    z = np.linspace(-1, 1, 12).astype(np.float32)
    text = (HEAD + 'Material "plastic" "rgb Kd" [0.5 0.25 0.125]\n' + ti.loopsubdiv_text(P, I, 2, ' "bool twosided" "false"')
            + 'AttributeBegin\nTranslate 0 2 0\nScale 2 2 -1\n' + ti.nurbs_text(kw) + 'AttributeEnd\n'
            + 'AttributeBegin\nReverseOrientation\n' + ti.heightfield_text(4, 3, z) + 'AttributeEnd\nWorldEnd\n')
    ps = capi.ParsedScene(text=text)
    sb = scenes.SceneBuilder()
    sb.material_plastic(Kd=(0.5, 0.25, 0.125))
    sb.shape_loopsubdiv(P, I, levels=2, twosided=False)
    t = scenes.transform_mul(scenes.transform_translate(0, 2, 0), scenes.transform_scale(2, 2, -1))
    sb.shape_nurbs(kw["nu"], kw["nv"], kw["uorder"], kw["vorder"], kw["uknots"], kw["vknots"], Pw=kw["Pw"], diceu=kw["diceu"], dicev=kw["dicev"],
                   object_to_world=t[0], world_to_object=t[1])
    sb.reverse_orientation = True
    sb.shape_heightfield(4, 3, z)
    sd = sb.build()
    a, b = ps.desc, sd.desc
    assert (a.n_vertices, a.n_triangles, a.n_meshes) == (b.n_vertices, b.n_triangles, b.n_meshes)
    for field, w in (("P", 3), ("N", 3), ("UV", 2)):
        assert same(np.ctypeslib.as_array(getattr(a, field), (a.n_vertices * w,)), np.ctypeslib.as_array(getattr(b, field), (b.n_vertices * w,))), field
    for field in ("indices", "tri_mesh"):
        n = a.n_triangles * (3 if field == "indices" else 1)
        assert np.array_equal(np.ctypeslib.as_array(getattr(a, field), (n,)), np.ctypeslib.as_array(getattr(b, field), (n,))), field
    for i in range(a.n_meshes):
        ma, mb = a.meshes[i], b.meshes[i]
        assert (ma.flags, ma.area_light, ma.object) == (mb.flags, mb.area_light, mb.object), i
        assert bytes(a.materials[ma.material]) == bytes(b.materials[mb.material]), i
