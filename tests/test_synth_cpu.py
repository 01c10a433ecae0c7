"""The synthetic scenes of tests/synth.py on the CPU: a second anchor for the
expected values (the C oracle against the independent numpy restatement on
the same arrays: frame, hit buffer and visit counters), and the conditions
that make tests/test_gpu_synth.py mean something, asserted on the oracle
alone.  No test here needs a GPU."""
import numpy as np
import pytest

from tests import synth as S

F = np.float32


@pytest.fixture(autouse=True)
def _close_scenes(monkeypatch):
    """Closes every SynthScene a test made (the oracle's scene handles)."""
    made = []
    init = S.SynthScene.__init__

    def tracked(self, *args, **kw):
        init(self, *args, **kw)
        made.append(self)

    monkeypatch.setattr(S.SynthScene, "__init__", tracked)
    yield
    for sc in made:
        sc.close()


def _anchor(sc, mode=0, xform=None, shadow=False, what=""):
    """The C oracle equals the numpy restatement: frame, hit buffer, counters."""
    argb, hit, cnt = sc.oracle(mode, xform=xform, shadow=shadow)
    nargb, nhit, ncnt = sc.oracle_np(mode, xform=xform, shadow=shadow)
    assert (hit == nhit).all(), f"{what}: hit buffers differ at {np.flatnonzero(hit != nhit)[:5]}"
    assert (argb == nargb).all(), f"{what}: frames differ at {np.flatnonzero(argb != nargb)[:5]}"
    assert [int(x) for x in cnt[:5]] == [int(x) for x in ncnt], what
    return argb, hit, cnt


# ------------------------------------------------------------ second anchor

@pytest.mark.parametrize("n", S.SOUP_NS)
def test_anchor_soups(n):
    """soup(n) at every setting of the tiny-tree test: KD, KD with shadow
    rays, and the flat list."""
    for name, kw, xf in S.SETTINGS:
        sc = S.soup_scene(n, cam_kw=kw)
        _anchor(sc, 0, xf, what=f"soup {n} {name}")
        _anchor(sc, 0, xf, shadow=True, what=f"soup {n} {name} shadow")
        _anchor(sc, 1, xf, what=f"soup {n} {name} flat")  # (the flat list takes no transform: the same frame)
        sc.close()


@pytest.mark.parametrize("n", S.EDGE_NS)
def test_anchor_edge_soups(n):
    with S.SynthScene(*S.edge_soup(n, S.EDGE_SEED + n), S.W, S.H_) as sc:
        for name, _, xf in S.SETTINGS[:3]:
            for shadow in (False, True):
                _anchor(sc, 0, xf, shadow=shadow, what=f"edge soup {n} {name} shadow {shadow}")
        _anchor(sc, 1, what=f"edge soup {n} flat")


def test_anchor_copies():
    with S.SynthScene(*S.copies(*S.COPIES), S.W, S.H_) as sc:
        _anchor(sc, 0, what="copies")
        _anchor(sc, 1, what="copies flat")
        _anchor(sc, 0, shadow=True, what="copies shadow")


@pytest.mark.parametrize("w,h", S.GRID_FRAMES + ((33, 9),))
def test_anchor_grid(w, h):
    for name, kw, xf in S.grid_poses(w, h):
        sc = S.SynthScene(*S.grid(), w, h, cam_kw=kw)
        for shadow in (False, True):
            _anchor(sc, 0, xf, shadow=shadow, what=f"grid {w}x{h} {name} shadow {shadow}")
        sc.close()


def test_anchor_scale_sweep():
    for e in S.SCALE_EXPONENTS + (S.DENORMAL_EXPONENT,):
        sc = S.scaled_soup(e)
        _anchor(sc, 0, what=f"scale 2^{e}")
        _anchor(sc, 1, what=f"scale 2^{e} flat")
        sc.close()


def test_anchor_hand_made_trees():
    """Every variant at the identity (with shadow rays too) and under the two
    object transforms the GPU test renders it under."""
    (v, f), trees = S.tree_variants()
    for name, nodes in trees.items():
        with S.SynthScene(v, f, S.W, S.H_, nodes=nodes) as sc:
            _anchor(sc, 0, what=f"tree {name}")
            _anchor(sc, 0, shadow=True, what=f"tree {name} shadow")
            for xname, xf in S.TREE_XFS:
                _anchor(sc, 0, xf, what=f"tree {name} {xname}")


def test_anchor_threshold_triangles():
    for extra in (False, True):
        for flip in (False, True):
            for ulps in (-1, 0, 1):
                with S.SynthScene(*S.threshold_triangle(ulps, flip, extra), S.W, S.H_, cam_kw=S.THRESHOLD_CAM) as sc:
                    _anchor(sc, 0, what=f"threshold {ulps} {flip} {extra}")
                    _anchor(sc, 0, shadow=True, what=f"threshold {ulps} {flip} {extra} shadow")
                    _anchor(sc, 1, what=f"threshold {ulps} {flip} {extra} flat")


def test_anchor_frame_loop_scenes():
    for n in (1, 2):
        with S.soup_scene(n) as sc:
            _anchor(sc, 0, what=f"soup {n}")


# ------------------------------------------------- conditions on the oracle

def test_soups_have_hits_and_misses():
    """Measured hit pixels of soup(n, 100 + n) at 33x19 (627 pixels), n = 1,
    2, 3, 4, 5, 8, 9, 33, 257: 8, 17, 38, 22, 21, 54, 63, 253, 610.  The eye
    of the "inside" setting lies inside every root box from n = 2 on (n = 1
    has no box test: its root is a leaf); no ray enters such a box."""
    want = {1: 8, 2: 17, 3: 38, 4: 22, 5: 21, 8: 54, 9: 63, 33: 253, 257: 610}
    for n in S.SOUP_NS:
        sc = S.soup_scene(n)
        assert len(sc.nodes) == 2 * n - 1
        _, hit, cnt = sc.oracle(0)
        nh = int((hit >= 0).sum())
        assert 0 < nh < hit.size, n
        assert nh == want[n] == int(cnt[3]), (n, nh)
        if n == 1:
            assert sc.nodes["is_leaf"][0] == 1 and int(cnt[0]) == 0
            continue
        r, p = sc.nodes[0], S.INSIDE_EYE["pos"]
        assert r["x0"] < p[0] < r["x1"] and r["y0"] < p[1] < r["y1"] and r["z0"] < p[2] < r["z1"], n
        _, ihit, icnt = S.soup_scene(n, cam_kw=S.INSIDE_EYE).oracle(0)
        assert (ihit < 0).all() and int(icnt[0]) == hit.size and int(icnt[4]) == 0


def test_edge_soups_hold_the_cases():
    """The edge soups hold what their docstring says, in float32 bits, and
    still have hit and miss pixels (12: 50 hits, 257: 273 hits of 627), the
    same in the KD walk and in the flat list."""
    want = {12: 50, 257: 273}
    for n in S.EDGE_NS:
        v, f = S.edge_soup(n, S.EDGE_SEED + n)
        t = v[f]                                         # [n, 3, 3]
        assert (t[5, 2] == t[5, 0]).all() or (t[5, 0] == t[5, 1]).all() or (t[5, 1] == t[5, 2]).all()
        assert (t[7, :, 0] == 0).all()
        assert (t[9, :, 2] < -1).all()
        assert (t[11, :, 2] < -1).sum() == 1
        cr = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])[:, 2]
        assert (cr[np.arange(n) != 5] > 0).sum() >= 3 and (cr < 0).sum() >= 3  # both windings face the eye
        sc = S.SynthScene(v, f, S.W, S.H_)
        _, hit, _ = sc.oracle(0)
        nh = int((hit >= 0).sum())
        assert 0 < nh < hit.size and nh == want[n], (n, nh)
        assert (hit == sc.oracle(1)[1]).all()


def test_copies_tie_pixels():
    """copies(48, 3, seed 7) at 33x19: 253 hit pixels; on 68 of them the KD
    walk's winner (the first-visited copy, `w < d` strict) is not the
    flat list's (the lowest index), on 185 the two agree.  Every winner pair
    is two copies of one triangle: the same vertex bits."""
    sc = S.SynthScene(*S.copies(*S.COPIES), S.W, S.H_)
    _, kd, _ = sc.oracle(0)
    _, flat, _ = sc.oracle(1)
    assert ((kd >= 0) == (flat >= 0)).all()
    m = kd >= 0
    differ, agree = int((m & (kd != flat)).sum()), int((m & (kd == flat)).sum())
    assert differ >= 20 and agree >= 20, (differ, agree)
    assert (differ, agree) == (68, 185)
    assert (sc.pts[kd[m]] == sc.pts[flat[m]]).all()
    assert (kd[m] >= flat[m]).all()   # the flat winner is the lowest-indexed copy


def test_grid_zero_components_meet_zero_bounds():
    """grid() has 28 triangles.  Rays with a component of exactly +-0: 51 at
    33x19, 11 at 7x5, 1 at 1x1, none at 32x18 (the control); the same counts
    with the eye on the split planes x = -0.15, y = 0.17.  At either eye some
    interior node has a camera-relative box bound and an s1 or s2 of exactly
    zero on x and on y, the axes of the zero components."""
    v, f = S.grid()
    assert len(f) == 28
    want = {(33, 19): 51, (7, 5): 11, (1, 1): 1, (32, 18): 0}
    for (w, h), nz in want.items():
        for name, kw, _ in (S.grid_poses(w, h)[0], S.grid_poses(w, h)[3]):
            sc = S.SynthScene(v, f, w, h, cam_kw=kw)
            rays = sc.rays()
            zero = rays == 0
            assert int(zero.any(axis=1).sum()) == nz, (w, h, name)
            if (w, h) in ((33, 19), (7, 5)):
                assert nz >= 10
            if nz == 0:
                continue
            pos = [F(x) for x in (kw or S.default_cam(w, h))["pos"]]
            inner = sc.nodes[sc.nodes["is_leaf"] == 0]
            for axis, (lo, hi) in enumerate((("x0", "x1"), ("y0", "y1"))):
                assert zero[:, axis].any(), (w, h, name, axis)
                cut = inner["cut_flag"] % 3 == axis
                assert ((inner[lo] - pos[axis] == 0) | (inner[hi] - pos[axis] == 0)).any(), (name, axis)
                assert ((inner["s1"][cut] - pos[axis] == 0) | (inner["s2"][cut] - pos[axis] == 0)).any(), (name, axis)
    kw = S.grid_eye_on_split(33, 19)
    assert kw["pos"][0] != 0.0 and kw["pos"][1] != float(F(0.1))


def test_scale_sweep_crosses_the_thresholds():
    """soup(16, seed 6) scaled with its camera by 2^e at 33x19, measured on
    the oracle (hit pixels; interior visits, leaf visits, descents):
        e = 0, 7, -8, -20, -21: 128 hits; 4092, 1391, 3598
        e = -22: 125   e = -23: 111   e = -24: 73   (same visit counters)
        e = -25, -26, -40: 0 hits, same visit counters
        e = -50: 0; 4986, 2099, 3973    e = -53: 0; 7658, 4458, 5996
        e = -56: 0; 9401, 9876, 9325
    The hits go with the determinant f ~ area * 2^2e falling below 1e-16
    (the reference's (double)f < 1e-16); from 2^-50 on the box coordinates
    are of the size of 1e-16 and the entry and ordering tests change the
    walk.  (soup(16, seed 16) has a single exponent between all hits and
    none; nearly every other seed has three, seed 6 among them.)"""
    res = {}
    for e in (0,) + S.SCALE_EXPONENTS:
        _, hit, cnt = S.scaled_soup(e).oracle(0)
        res[e] = (int((hit >= 0).sum()), int(cnt[0]), int(cnt[1]), int(cnt[4]))
    assert res[-20][0] == res[0][0] == 128
    assert res[-20] == res[0] == res[7] == res[-8]
    assert res[-26][0] == 0
    between = [e for e in S.SCALE_EXPONENTS if 0 < res[e][0] < res[0][0]]
    assert len(between) >= 2 and [res[e][0] for e in (-22, -23, -24)] == [125, 111, 73], res
    assert len({res[e][1] for e in S.SCALE_EXPONENTS}) >= 3
    assert [res[e][1:] for e in (-40, -50, -53, -56)] == [(4092, 1391, 3598), (4986, 2099, 3973), (7658, 4458, 5996),
                                                          (9401, 9876, 9325)], res


def test_denormal_scale():
    """At 2^-60 the primary ray's sum of squares (the argument of the 21-step
    inverse square root) is a denormal float at every pixel, while every ray
    component is finite and the rays are bit for bit those of the unscaled
    camera.  A kernel that flushed f32 denormals would see 0 there and
    produce infinite or NaN rays: this is the scene that tells."""
    sc = S.scaled_soup(S.DENORMAL_EXPONENT)
    cam = sc.ocam()
    tiny = np.finfo(F).tiny
    for iy in range(sc.h):
        for ix in range(sc.w):
            c = [F(F(F(cam.n_mod[k]) + F(F(cam.u_mod[k]) * F(ix))) + F(F(cam.v_mod[k]) * F(iy))) for k in range(3)]
            s = F(F(F(c[0] * c[0]) + F(c[1] * c[1])) + F(c[2] * c[2]))
            assert 0 < s < tiny, (ix, iy, s)
    rays = sc.rays()
    assert np.isfinite(rays).all()
    assert np.abs(np.linalg.norm(rays.astype(np.float64), axis=1) - 1).max() < 1e-3
    _, hit, cnt = sc.oracle(0)
    assert (hit < 0).all() and int(cnt[0]) == 9405


def test_hand_made_trees_change_the_walk():
    """The variants of soup(33)'s tree differ from the built tree where they
    are meant to: a shrunk leaf box changes nothing (the walk never tests a
    leaf's box), the others change the visit counters.  tree_variants itself
    asserts which variants keep s1 / s2 equal to the children's bounds."""
    (v, f), trees = S.tree_variants()
    cnt = {}
    for name, nodes in trees.items():
        _, hit, c = S.SynthScene(v, f, S.W, S.H_, nodes=nodes).oracle(0)
        cnt[name] = ([int(x) for x in c[:5]], hit)
    for name in ("shrunk", "shrunk_split"):
        assert cnt[name][0] == cnt["built"][0] and (cnt[name][1] == cnt["built"][1]).all()
    for name in ("swapped", "inflated", "inflated_split", "shrunk_interior"):
        assert cnt[name][0] != cnt["built"][0], name


def test_threshold_triangles_sit_on_the_threshold():
    """The centre ray of the 33x19 frame of THRESHOLD_CAM is exactly (0, 0, 1)
    and the sliver's determinant for it is +-(0xE69595 + ulps) * 2^-77: at
    ulps = 0 the smallest float >= 1e-16, which the reference keeps, at -1 the
    largest below, which it rejects.  So the centre pixel (313) is hit at 0
    and +1 and missed at -1, in both windings, in the KD walk and the flat
    list, alone (leaf root) and with three more triangles (24 other hit
    pixels): a threshold off by one ulp in either direction changes a pixel."""
    eps_f = np.array([S.EPS_F_BITS], np.uint32).view(F)[0]
    below = np.array([S.EPS_F_BITS - 1], np.uint32).view(F)[0]
    assert np.float64(eps_f) >= 1e-16 > np.float64(below)
    centre = (S.H_ // 2) * S.W + S.W // 2
    for extra in (False, True):
        for flip in (False, True):
            for ulps in (-1, 0, 1):
                v, f = S.threshold_triangle(ulps, flip, extra)
                sc = S.SynthScene(v, f, S.W, S.H_, cam_kw=S.THRESHOLD_CAM)
                assert sc.rays()[centre].tobytes() == np.array([0, 0, 1], F).tobytes()
                p = sc.pts[0].reshape(3, 3)
                e1, e2 = p[1] - p[0], p[2] - p[0]
                det = F(F(F(-e2[1]) * e1[0]) + F(e2[0] * e1[1]))   # ((0,0,1) x e2) . e1
                want_bits = S.EPS_F_BITS + ulps
                assert np.array([abs(det)], F).view(np.uint32)[0] == want_bits, (ulps, flip)
                for mode in (0, 1):
                    _, hit, _ = sc.oracle(mode)
                    assert (hit[centre] == 0) == (ulps >= 0), (extra, flip, ulps, mode)
                    assert int((hit >= 0).sum()) == (24 if extra else 0) + (ulps >= 0)
    dets = set()
    for flip in (False, True):
        p = S.SynthScene(*S.threshold_triangle(0, flip), S.W, S.H_, cam_kw=S.THRESHOLD_CAM).pts[0].reshape(3, 3)
        e1, e2 = p[1] - p[0], p[2] - p[0]
        dets.add(float(F(F(F(-e2[1]) * e1[0]) + F(e2[0] * e1[1]))) > 0)
    assert dets == {True, False}   # one winding's determinant is +1e-16, the other's -1e-16


# ------------------------------------------- the light's side and the materials

LIGHT_XFS = (("identity", None),) + S.TREE_XFS


@pytest.mark.parametrize("pose", S.LIGHT_POSE_NAMES)
def test_anchor_light_poses(pose):
    """soup(65) from every eye of light_poses(): without shadow rays, and with
    them at the identity and under the two object transforms the GPU test
    renders."""
    with S.light_scene(pose) as sc:
        _anchor(sc, 0, what=f"light {pose}")
        for name, xf in LIGHT_XFS:
            _anchor(sc, 0, xf, shadow=True, what=f"light {pose} {name} shadow")


@pytest.mark.parametrize("which", S.LIGHT_PLANES)
@pytest.mark.parametrize("w,h", S.LIGHT_PLANE_FRAMES)
def test_anchor_light_planes(w, h, which):
    with S.light_planes_scene(which, w, h) as sc:
        for name, xf in S.LIGHT_PLANE_XFS:
            for shadow in (False, True):
                _anchor(sc, 0, xf, shadow=shadow, what=f"light planes {which} {w}x{h} {name} shadow {shadow}")


def test_anchor_light_tie():
    with S.SynthScene(*S.light_tie(), S.W, S.H_, cam_kw=S.THRESHOLD_CAM) as sc:
        for shadow in (False, True):
            _anchor(sc, 0, shadow=shadow, what=f"light tie shadow {shadow}")


def test_anchor_light_on_triangle():
    v, f, kw = S.light_on_triangle()
    with S.SynthScene(v, f, S.W, S.H_, cam_kw=kw) as sc:
        for shadow in (False, True):
            _anchor(sc, 0, shadow=shadow, what=f"light on triangle shadow {shadow}")


@pytest.mark.parametrize("table", S.MATERIAL_TABLES)
def test_anchor_materials(table):
    """Per-triangle radiance through both oracles: KD, KD with shadow rays,
    the flat list, and the two layers of the composite test."""
    with S.material_scene(table) as sc:
        _anchor(sc, 0, what=f"{table}")
        _anchor(sc, 0, shadow=True, what=f"{table} shadow")
        _anchor(sc, 1, what=f"{table} flat")
    for n, tname, xf in S.OVER_LAYERS:
        with S.material_scene(tname, n) as sc:
            _anchor(sc, 0, xf, what=f"over layer {tname} {n}")


def _shadowed(sc, xform=None):
    """(hit mask, shadowed mask) of the oracle: a shadowed pixel is a hit
    whose colour the shadow pass zeroes (and that was not zero before)."""
    a0, hit, _ = sc.oracle(0, xform=xform)
    a1, _, _ = sc.oracle(0, xform=xform, shadow=True)
    m = hit >= 0
    assert (a0[m] != 0).all() and (a1[~m] == a0[~m]).all() and ((a1 == a0) | (a1 == 0)).all()
    return m, m & (a1 == 0)


def test_light_octants_hold_their_sign():
    """The eight octant eyes: every hit pixel's shadow ray has the signs of o
    on all three axes, strictly (no component below 0.33 in magnitude).
    Measured (hit, shadowed pixels of 627) for o = (x, y, z) in the order of
    LIGHT_OCTANTS: nnn 341, 155; pnn 309, 86; npn 353, 133; ppn 343, 110; nnp
    351, 117; pnp 321, 91; npp 350, 140; ppp 329, 44."""
    want = dict(nnn=(341, 155), pnn=(309, 86), npn=(353, 133), ppn=(343, 110), nnp=(351, 117), pnp=(321, 91),
                npp=(350, 140), ppp=(329, 44))
    assert len(S.LIGHT_OCTANTS) == 8 == len({tuple(o) for o in S.LIGHT_OCTANTS})
    for o in S.LIGHT_OCTANTS:
        name = S._pose_name(o)
        sc = S.light_scene(name)
        m, sh = _shadowed(sc)
        pix, dirs, _ = S.shadow_rays(sc)
        assert (pix == np.flatnonzero(m)).all()
        assert (np.sign(dirs) == np.array(o, F)).all(), name
        assert np.abs(dirs).min() > 0.33
        assert (int(m.sum()), int(sh.sum())) == want[name], (name, int(m.sum()), int(sh.sum()))
        assert sh.sum() >= 20 and (m & ~sh).sum() >= 20


def _mixed_runs(pix, comp, w, width):
    """The aligned runs of `width` pixels of one row (x0 a multiple of width)
    in which hit pixels with comp > 0 and with comp < 0 both occur."""
    runs = {}
    for p, c in zip(pix, comp):
        runs.setdefault((int(p) // w, (int(p) % w) // width), set()).add(bool(c > 0))
    return [k for k, s in runs.items() if len(s) == 2]


def test_light_straddles_mix_signs_inside_a_unit():
    """The six straddle eyes: on each straddled axis (o = 0) both signs occur,
    and they occur together inside aligned runs of 8 pixels of one row, which
    unit_pixel (rt_kernels_impl.h) gives to one wave's unit at 8, 16 and 32
    rays (8 columns from a multiple of 8, rays / 8 rows), and inside aligned
    runs of 4, the half rows of a split 8-ray unit (kd3_block): such waves
    hold rays of several octants.  On the other axes the sign is o's.  No
    component is zero.  Measured per pose (hit, shadowed; per straddled axis
    negative / positive pixels, mixed runs of 8, of 4):
        zpp 349, 108; x 183 / 166, 19, 19
        pzn 339, 124; y 178 / 161, 23, 19
        npz 332, 129; z 200 / 132, 15, 13
        zzp 332,  84; x 180 / 152, 21, 19; y 191 / 141, 11, 9
        znz 322, 108; x 170 / 152, 25, 22; z 190 / 132, 16, 15
        pzz 324,  97; y 170 / 154, 23, 23; z 172 / 152, 17, 15"""
    want = dict(zpp=(349, 108), pzn=(339, 124), npz=(332, 129), zzp=(332, 84), znz=(322, 108), pzz=(324, 97))
    for o in S.LIGHT_STRADDLES:
        name = S._pose_name(o)
        sc = S.light_scene(name)
        m, sh = _shadowed(sc)
        pix, dirs, _ = S.shadow_rays(sc)
        assert (dirs != 0).all()
        assert (int(m.sum()), int(sh.sum())) == want[name], (name, int(m.sum()), int(sh.sum()))
        assert sh.sum() >= 20 and (m & ~sh).sum() >= 20
        for k in range(3):
            if o[k] != 0:
                assert (np.sign(dirs[:, k]) == o[k]).all(), (name, k)
                continue
            assert (dirs[:, k] < 0).sum() >= 20 and (dirs[:, k] > 0).sum() >= 20, (name, k)
            assert len(_mixed_runs(pix, dirs[:, k], S.W, 8)) >= 1, (name, k)
            assert len(_mixed_runs(pix, dirs[:, k], S.W, 4)) >= 1, (name, k)
        r = sc.nodes[0]   # the light (eye + 2) within the root box's range exactly on the straddled axes
        light = [F(F(p) + F(2)) for p in sc.cam_kw["pos"]]
        inside = [bool(r[lo] < light[k] < r[hi]) for k, (lo, hi) in enumerate((("x0", "x1"), ("y0", "y1"), ("z0", "z1")))]
        assert inside == [c == 0 for c in o], name


def test_light_inside_the_root_box():
    """The "inside" eye: the light lies inside soup(65)'s root box on every
    axis, off its centre; both signs occur on every axis (x 35 / 291, y 249 /
    77, z 134 / 192 negative / positive of 326 hit pixels), so no axis can
    prove the shadow walk.  No pixel is shadowed, at this or at any other
    light inside the box: every slab's entry parameter of the root is
    negative there and the reference's walk enters no box that holds its
    ray's origin (maxt0 > -1e-16, TD/Trixel.cu:146; edge_soup()'s docstring
    has the same for the eye), so each shadow walk ends at the root, 326
    interior visits and no descent.  (An inside light that shadows a pixel
    does not exist for this walk; the straddle eyes are the ones with a light
    within the box's range on some axes and shadows.)"""
    sc = S.light_scene("inside")
    m, sh = _shadowed(sc)
    pix, dirs, _ = S.shadow_rays(sc)
    assert int(m.sum()) == 326
    for k, (neg, pos) in enumerate(((35, 291), (249, 77), (134, 192))):
        assert (int((dirs[:, k] < 0).sum()), int((dirs[:, k] > 0).sum())) == (neg, pos), k
    r = sc.nodes[0]
    light = [F(F(p) + F(2)) for p in sc.cam_kw["pos"]]
    assert r["x0"] < light[0] < r["x1"] and r["y0"] < light[1] < r["y1"] and r["z0"] < light[2] < r["z1"]
    assert int(sh.sum()) == 0
    c0, c1 = sc.oracle(0)[2], sc.oracle(0, shadow=True)[2]
    assert int(c1[0]) - int(c0[0]) == 326 and int(c1[4]) == int(c0[4]) and int(c1[1]) == int(c0[1])


def test_light_planes_zero_components():
    """light_planes() from THRESHOLD_CAM: hit pixels whose shadow ray has a
    component of exactly +-0, per axis x / y / z, and how many of those
    pixels the oracle shadows / leaves lit:
        "z"    33x19 338 hits,  0 / 0 / 156, 135 / 21    32x18 288,  0 / 0 / 140, 122 / 18
               7x5    18 hits,  0 / 0 / 6,     5 / 1     1x1 no hit
        "xyz"  33x19 350 hits, 10 / 0 / 156, 135 / 31    32x18 305, 11 / 0 / 140, 122 / 29
               7x5    18 hits,  0 / 0 / 6,     5 / 1     1x1 no hit
        "xz"   33x19 359 hits, 16 / 0 / 156, 135 / 37    32x18 316, 16 / 0 / 140, 122 / 34
               7x5    18 hits,  0 / 0 / 6,     5 / 1     1x1 no hit
    (32x18 is no control here: a third data point.  The wall in y = 2 lies
    above the frame; it is there so that no axis proves the shadow walk.)
    The walls' boxes have equal bounds on their plane's axis, the light's
    coordinate: relative to the light exact zeros."""
    want = {("z", 33, 19): (338, (0, 0, 156), 135, 21), ("z", 32, 18): (288, (0, 0, 140), 122, 18),
            ("z", 7, 5): (18, (0, 0, 6), 5, 1), ("z", 1, 1): (0, (0, 0, 0), 0, 0),
            ("xyz", 33, 19): (350, (10, 0, 156), 135, 31), ("xyz", 32, 18): (305, (11, 0, 140), 122, 29),
            ("xyz", 7, 5): (18, (0, 0, 6), 5, 1), ("xyz", 1, 1): (0, (0, 0, 0), 0, 0),
            ("xz", 33, 19): (359, (16, 0, 156), 135, 37), ("xz", 32, 18): (316, (16, 0, 140), 122, 34),
            ("xz", 7, 5): (18, (0, 0, 6), 5, 1), ("xz", 1, 1): (0, (0, 0, 0), 0, 0)}
    for which in S.LIGHT_PLANES:
        v, f = S.light_planes(which)
        assert len(f) == {"z": 25, "xz": 27, "xyz": 29}[which] <= 257
        for w, h in S.LIGHT_PLANE_FRAMES:
            sc = S.light_planes_scene(which, w, h)
            m, sh = _shadowed(sc)
            pix, dirs, _ = S.shadow_rays(sc)
            zero = dirs == 0
            anyz = zero.any(axis=1)
            got = (int(m.sum()), tuple(int(x) for x in zero.sum(axis=0)), int((anyz & sh[pix]).sum()),
                   int((anyz & ~sh[pix]).sum()))
            assert got == want[which, w, h], (which, w, h, got)
            if (w, h) == (33, 19):
                assert anyz.sum() >= 100 and got[2] >= 20 and got[3] >= 20
                if which != "z":
                    assert (zero.sum(axis=0) > 0).sum() >= 2
            r = sc.nodes[0]
            assert (r["x1"] < 2) == (which == "z") and r["z0"] < 1 < r["z1"]
            assert (r["y1"] < 2) == (which != "xyz")         # "xz": x fails, the proof holds on y
            if which == "xyz":
                assert r["x0"] < 2 <= r["x1"] and r["y0"] < 2 <= r["y1"]
        leaf = sc.nodes[sc.nodes["is_leaf"] == 1]
        assert ((leaf["z0"] == 1) & (leaf["z1"] == 1)).sum() == 24
        if "x" in which:
            assert ((leaf["x0"] == 2) & (leaf["x1"] == 2)).sum() == 2
        if which == "xyz":
            assert ((leaf["y0"] == 2) & (leaf["y1"] == 2)).sum() == 2


def test_light_on_triangle_walks_short_segments():
    """light_on_triangle(): the replaced triangle lies in the plane z = the
    light's z with the light at the midpoint of its edge in x = the light's
    x; both coordinates are the root box's x0 and z0 bit for bit, and every
    other triangle lies beyond them.  Measured at 33x19: 222 hit pixels, 19 of
    them the triangle's, which are the 19 smallest Lmax of the frame (0.0283
    to 0.135; the largest is 1.132).  Every one of the 222 shadow walks enters
    the root and visits a leaf (the 19 in-plane ones one to three leaves each,
    their own triangle's among them); 13 pixels are shadowed, 209 lit, none
    of the triangle's own (no triangle lies in its plane between it and the
    light)."""
    v, f, kw = S.light_on_triangle()
    light = np.array([F(F(p) + F(2)) for p in kw["pos"]], F)
    t = v[f[S.LIGHT_TRI]]
    assert (t[:, 2] == light[2]).all() and (t[:2, 0] == light[0]).all() and t[2, 0] > light[0]
    assert t[0, 1] < light[1] < t[1, 1]                       # the light on the edge t0-t1
    others = np.delete(v.reshape(-1, 3, 3), S.LIGHT_TRI, axis=0)
    assert (others[..., 0] > light[0]).all() and (others[..., 2] > light[2]).all()
    sc = S.SynthScene(v, f, S.W, S.H_, cam_kw=kw)
    r = sc.nodes[0]
    assert r["x0"] == light[0] and r["z0"] == light[2] and r["y0"] < light[1] < r["y1"]
    m, sh = _shadowed(sc)
    _, hit, _ = sc.oracle(0)
    pix, _, lmax = S.shadow_rays(sc)
    vpix, occ, desc, leaf = S.shadow_visits(sc)
    assert (vpix == pix).all() and (occ == sh[pix]).all()
    mine = hit[pix] == S.LIGHT_TRI
    assert (int(m.sum()), int(mine.sum()), int(sh.sum())) == (222, 19, 13)
    assert lmax[mine].max() < lmax[~mine].min() and lmax.min() == lmax[mine].min()
    assert (desc > 0).all() and (leaf > 0).all()              # every shadow walk descends to leaves
    assert set(leaf[mine].tolist()) == {1, 2, 3} and not occ[mine].any()
    assert sh.sum() >= 1 and (m & ~sh).sum() >= 1
    c0, c1 = sc.oracle(0)[2], sc.oracle(0, shadow=True)[2]
    assert int(c1[4]) - int(c0[4]) == int(desc.sum()) and int(c1[1]) - int(c0[1]) == int(leaf.sum())
    assert (round(float(lmax.min()), 4), round(float(lmax[mine].max()), 3)) == (0.0283, 0.135)
    assert lmax.min() == F(0.028286124) and 1.13 < lmax.max() < 1.14


def test_materials_vary_the_frame():
    """soup(65) at the default view, 331 hit pixels.  materials(65): no two
    triangles share a channel value; the frame differs from the one-material
    frame at all 331 hit pixels, and at 247 of them the largest channel is not
    green.  EDGE_RAD cycled: every one of its 11 rows is the material of some
    hit pixel; the frame's hit pixels hold 395 channel bytes of 0, 460 of 255
    and 138 strictly between (the all-negative row and the infinities take
    to_u8's >= 256 branch, NaN and negative ratios its first), and at 262 hit
    pixels the largest byte is not green's alone."""
    base = S.soup_scene(S.LIGHT_N)
    b, bhit, _ = base.oracle(0)
    m = bhit >= 0
    assert int(m.sum()) == 331
    g = (b[m] >> 8) & 255
    assert (g == 255).all()                      # the one material: green is 255 at every lit pixel
    got = {}
    for table in S.MATERIAL_TABLES:
        sc = S.material_scene(table)
        a, hit, _ = sc.oracle(0)
        assert (hit == bhit).all() and (a >> 24 == 0).all() and (a[~m] == b[~m]).all()
        by = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], 1)[m]
        got[table] = (int((a != b)[m].sum()), int((by == 0).sum()), int((by == 255).sum()),
                      int(((by > 0) & (by < 255)).sum()), int((by.argmax(1) != 1).sum()))
        if table == "edge":
            assert set((hit[m] % len(S.EDGE_RAD)).tolist()) == set(range(len(S.EDGE_RAD)))
            assert (sc.rad.view(np.uint32) == S.EDGE_RAD.view(np.uint32)[np.arange(S.LIGHT_N) % 11]).all()
    assert got["materials"][0] >= m.sum() // 2 and got["materials"][4] >= 1
    assert got["edge"][1] >= 1 and got["edge"][2] >= 1 and got["edge"][3] >= 1 and got["edge"][4] >= 1
    assert got == {"materials": (331, 0, 331, 662, 247), "edge": (331, 395, 460, 138, 262)}, got


def test_over_layers_interleave():
    """The two layers of test_materials_over (soup(65) with materials, soup(33)
    with EDGE_RAD, rotated): pixels where only the base, only the layer, both
    with the layer nearer, both with the base nearer hit, exact ties, neither:
    237, 91, 58, 36, 0, 205 of 627."""
    from tests.test_over_cpu import hit_classes
    frames = []
    for n, tname, xf in S.OVER_LAYERS:
        sc = S.material_scene(tname, n)
        planes, hit = sc.np_planes(xf)
        assert (hit.reshape(-1) == sc.oracle(0, xform=xf)[1]).all()
        frames.append((hit, planes[0]))
    cls = hit_classes(frames[0][0], frames[0][1], frames[1][0], frames[1][1])
    assert cls[0] >= 20 and cls[1] >= 5 and cls[2] >= 20 and cls[3] >= 20 and cls[4] == 0, cls
    assert cls == S.OVER_CLASSES, cls


def test_light_tie_entry_equals_lmax():
    """light_tie() at 33x19: 405 hit pixels, all on the wall.  The root box's
    entry parameter for the shadow ray equals Lmax bit for bit at 48 of them,
    is below it at 58 (the walk enters the root) and above it at 299 (it does
    not): the oracle's descents of the shadow pass are the 58, so entering at
    maxt0 <= Lmax instead of maxt0 < Lmax would count 106."""
    sc = S.SynthScene(*S.light_tie(), S.W, S.H_, cam_kw=S.THRESHOLD_CAM)
    m, sh = _shadowed(sc)
    pix, dirs, lmax = S.shadow_rays(sc)
    t0 = S.root_entry(sc, dirs)
    got = (int(m.sum()), int((t0 == lmax).sum()), int((t0 < lmax).sum()), int((t0 > lmax).sum()))
    assert got[1] >= 20 and got[2] >= 20 and got[3] >= 20, got
    c0, c1 = sc.oracle(0)[2], sc.oracle(0, shadow=True)[2]
    assert int(c1[0]) - int(c0[0]) >= got[0]                 # every shadow ray visits the root
    assert int(c1[4]) - int(c0[4]) == got[2], (got, c0, c1)  # and descends only where maxt0 < Lmax
    assert got == (405, 48, 58, 299), got


# ------------------------------------------- the deferred shadow pass (rt_shadow_over)
# What tests/test_gpu_xshadow_synth.py's scenes hold, on the two oracles alone.

def _np():
    from oracle import np_oracle as N
    from tests import test_xshadow_cpu as X
    return N, X


def _twin(sc, xf):
    """The numpy reference of sc's object at xf under its twin: cross_shadow of
    two objects of the same mesh, tree and transform, with each pass's
    counters -> (argb, hit, planes, classes), [base's counters, twin's]."""
    N, X = _np()
    P, cam = S.np_scene(sc), sc.np_camera()
    Xf = N.IDENT if xf is None else np.asarray(xf, F)
    tr = X.trace_object(P, cam, Xf, np.arange(sc.w * sc.h))
    cnt = [[0] * 5, [0] * 5]
    return X.cross_shadow(P, cam, [Xf, Xf], traced=[tr, tr], cnt=cnt), cnt


@pytest.mark.parametrize("name", list(S.TWIN_CASES))
def test_twin_pass_walks_the_fused_corpus(name):
    """A twin (the same mesh, tree and transform from a second camera, hit
    base = the triangle count) owns no pixel of the composite (the depth test
    is strict), so its pass walks exactly the hit points of the fused shadow
    render, each as a foreign pixel: nothing excluded.  Its shadow set is the
    self pass's, and both frames are the C oracle's shadow frame, with the
    numpy reference as the judge.  Counters: the oracle's shadow render minus
    its plain render is exact for both passes on [0], [1], [4] (the DFS does
    not depend on the exclusion) and for the self pass on [2]; the twin's
    accept events [2] are no fewer (it excludes nothing)."""
    make, xfs = S.TWIN_CASES[name]
    sc = make()
    for xname, xf in xfs:
        (argb, hit, _, cls), cnt = _twin(sc, xf)
        assert (cls["owner"] != 1).all(), (name, xname)
        assert (cls["by"][0] == cls["by"][1]).all(), (name, xname, np.flatnonzero(cls["by"][0] != cls["by"][1])[:5])
        c0, c1 = sc.oracle(0, xform=xf)[2], sc.oracle(0, xform=xf, shadow=True)
        assert (hit == c1[1]).all() and (argb == c1[0]).all(), (name, xname, np.flatnonzero(argb != c1[0])[:5])
        diff = [int(c1[2][k]) - int(c0[k]) for k in range(5)]
        assert [cnt[0][k] for k in (0, 1, 2, 4)] == [diff[k] for k in (0, 1, 2, 4)], (name, xname, cnt, diff)
        assert [cnt[1][k] for k in (0, 1, 4)] == [diff[k] for k in (0, 1, 4)] and cnt[1][2] >= diff[2], (name, xname, cnt)
        S.pass_check(argb, cnt[1], c1[0], diff, (name, xname))


def test_xshadow_scale_exponents():
    """scaled_soup(e)'s shadow frame has a shadowed pixel at 2^7 alone of
    SCALE_EXPONENTS (1 of 128 hit pixels; 21 at 2^0, none from 2^-8 down: the
    light stays 2 away from the eye on every axis while the scene shrinks)."""
    got = {}
    for e in S.SCALE_EXPONENTS:
        m, sh = _shadowed(S.scaled_soup(e))
        got[e] = int(sh.sum())
    assert tuple(e for e in S.SCALE_EXPONENTS if got[e] > 0) == S.XSHADOW_SCALE_EXPONENTS, got
    assert got[7] == 1


@pytest.mark.parametrize("pose", S.LIGHT_POSE_NAMES)
def test_xshadow_two_soups_classes(pose):
    """soup(65) from light_scene(pose)'s eye under itself at the two offsets of
    XSHADOW_OFFSETS: layer pixels shadowed by the base only, by both, base
    pixels shadowed by the layer only, by both (XSHADOW_CLASSES).  Every class
    holds at least 2 pixels at every pose and offset but "inside", whose light
    shadows nothing (the control)."""
    _, X = _np()
    for k in range(len(S.XSHADOW_OFFSETS)):
        got = X.class_counts(X.pair_want(pose, k)[0][3])
        assert (min(got) >= 2) if pose != "inside" else (got == (0, 0, 0, 0)), (pose, k, got)
        assert got == S.XSHADOW_CLASSES[pose, k], (pose, k, got)


def test_xshadow_tiny_occluders():
    """soup(n) at XSHADOW_TINY_OFFSET over soup(65), and soup(65) at that
    offset over soup(n), from the default camera: the small soup as the layer
    shadows a base pixel at every n (n = 1, a leaf root: 2 pixels)."""
    _, X = _np()
    for n in S.SOUP_NS:
        over, under = (X.class_counts(X.tiny_want(n, layer)[0][3]) for layer in (True, False))
        assert over[2] + over[3] >= 1, (n, over)
        assert (over, under) == S.XSHADOW_TINY[n], (n, over, under)
    assert S.XSHADOW_TINY[1][0][2] + S.XSHADOW_TINY[1][0][3] == 2


def _foreign_segments(want, Ps, traced, B):
    """Pass B's foreign pixels (hit, not B's own) and their segment classes."""
    hit, owner = want[1], want[3]["owner"]
    idx = np.flatnonzero((hit >= 0) & (owner != B))
    d = want[2][0].view(F)[idx]
    return idx, S.segment_classes(Ps[B], d, [traced[B][3][int(j)] for j in idx])


def test_xshadow_segments_end_before_inside_and_beyond_the_box():
    """The foreign pixels of the two-soup scenes by where their shadow segment
    ends relative to the occluder's root box: before it (root entry at or
    beyond Lmax: no descent), inside it, beyond it.  Each class occurs over
    the poses; a pixel of the first class is never shadowed."""
    total = np.zeros(3, np.int64)
    for pose in S.LIGHT_POSE_NAMES:
        _, X = _np()
        want, Ps, traced = X.pair_want(pose, 0)
        for B in (0, 1):
            idx, cls = _foreign_segments(want, Ps, traced, B)
            total += np.bincount(cls[cls >= 0], minlength=3)
            assert not want[3]["by"][B][idx[cls == 0]].any(), (pose, B)
    print("segments ending before / inside / beyond the occluder's root box:", total)
    assert (total >= 1).all(), total


def _faulty_pass(want, Ps, traced, B, scale=None, le=False, exclude_foreign=False):
    """Object B's pass over the composite `want` (cross_shadow's result)
    restated with one fault of a wrong kernel: scale, the Lmax factor; le, a
    box entered where maxt0 <= Lmax; exclude_foreign, the own-triangle
    exclusion applied to a foreign pixel (its owner's triangle index read as
    one of B's).  -> (argb, counters)."""
    N, _ = _np()
    scale = N.SHADOW_SCALE if scale is None else F(scale)
    argb, hit, owner = want[0].copy(), want[1], want[3]["owner"]
    bases = np.concatenate([[0], np.cumsum([len(p["e1"]) for p in Ps])])
    d0 = want[2][0].view(F)
    cnt = [0] * 5
    argb[want[3]["by"].any(0)] = 1       # (the other passes' shadows are not this pass's business)
    with np.errstate(all="ignore"):
        for j in np.flatnonzero(hit >= 0):
            rmi = int(hit[j] - bases[owner[j]]) if owner[j] == B or exclude_foreign else -1
            r, od = traced[B][3][j]
            sv = [F(F(F(d0[j] * r[k]) - od[k]) - F(2)) for k in range(3)]
            L2 = F(F(F(sv[0] * sv[0]) + F(sv[1] * sv[1])) + F(sv[2] * sv[2]))
            lmax = F(F(np.sqrt(np.float64(L2))) * scale)
            occ = [False]

            def leaf(t, u, v, w):
                if t != rmi and N._mt_accept(u, v, w, lmax):
                    cnt[2] += 1
                    occ[0] = True

            N._walk(Ps[B], list(N.dev_normalize(*sv)), (F(-2), F(-2), F(-2)), leaf,
                    lim=np.nextafter(lmax, F(np.inf)) if le else lmax, cnt=cnt)
            if occ[0]:
                argb[j] = 0
    return argb, cnt


def test_a_wrong_kernel_fails_the_comparison():
    """Three faults a pass could have, restated in numpy and fed to the
    comparison the GPU tests use (synth.pass_check): each is caught by a scene,
    and the faultless restatement passes it.
      the Lmax factor 1 instead of 1 - 2^-10: a twin pass finds each hit
        point's own triangle (soup(33): frame);
      the own-triangle exclusion applied to foreign pixels: the two soups of
        "pnp" (frame);
      a box entered at maxt0 <= Lmax: light_tie(), whose frame is the same and
        whose descents are 106 instead of 58."""
    N, X = _np()

    def one(want, Ps, traced, B, **fault):
        ok = _faulty_pass(want, Ps, traced, B)
        assert (ok[0] == 0).sum() == want[3]["by"][B].sum()
        bad = _faulty_pass(want, Ps, traced, B, **fault)
        S.pass_check(ok[0], ok[1], ok[0], ok[1])
        with pytest.raises(AssertionError):
            S.pass_check(bad[0], bad[1], ok[0], ok[1])
        return ok, bad

    def twin(sc):
        P, cam = S.np_scene(sc), sc.np_camera()
        tr = X.trace_object(P, cam, N.IDENT, np.arange(sc.w * sc.h))
        return X.cross_shadow(P, cam, [N.IDENT, N.IDENT], traced=[tr, tr]), [P, P], [tr, tr]

    ok, bad = one(*twin(S.soup_scene(33)), 1, scale=1.0)
    assert (bad[0] != ok[0]).sum() >= 20
    ok, bad = one(*X.pair_want("pnp", 0), 0, exclude_foreign=True)
    assert (bad[0] != ok[0]).any()
    sc = S.SynthScene(*S.light_tie(), S.W, S.H_, cam_kw=S.THRESHOLD_CAM)
    ok, bad = one(*twin(sc), 1, le=True)
    assert (bad[0] == ok[0]).all() and (ok[1][4], bad[1][4]) == (58, 106)


# ------------------------------------------- translated walks on exact split values
# What tests/test_gpu_synth.py's translated grid cases hold, on the two oracles.

def test_xl_offsets_are_split_planes_of_the_built_tree():
    """What _xl_cases says of grid()'s built tree, at every scale of the table:
    relative to the eye its x splits (s2) are 0, +-0.15, -0.2 and -0.3, its y
    splits 0 alone, with an s1 at 0.17 - 0.1, and its z splits lie at 1 (the
    tiles' plane; s == +1 at every pixel of an unmoved grid); the root box's
    near face is 0.4 in front of the eye (the z cases)."""
    for e in (0, 2, 3):
        sc = S.xl_grid(e)
        P = S.np_scene(sc)
        k = F(2.0) ** F(e)
        inner = [vx for vx in P["vox"] if not vx["leaf"]]
        s2 = [{float(vx["s2"]) for vx in inner if vx["cf"][axis] == 1} for axis in range(3)]
        assert s2[0] == {float(F(F(x) * k)) for x in (0, 0.15, -0.15, -0.2, -0.3)}, (e, s2)
        assert s2[1] == {0.0} and s2[2] == {float(k)}, (e, s2)
        assert float(F(F(F(0.17) * k) - F(F(0.1) * k))) in {float(vx["s1"]) for vx in inner if vx["cf"][1] == 1}
        assert P["vox"][0]["bo"][2] == F(F(F(-0.6) * k) - F(F(-1.0) * k))
    assert F(F(0.17) - F(0.1)) == F(np.float64(F(0.17)) - np.float64(F(0.1)))   # (an exact difference)


@pytest.mark.parametrize("name", list(S.XL_CASES))
def test_xl_case_reaches_its_classes(name):
    """Each case of XL_CASES at 33x19: the C oracle and the numpy restatement
    agree on frame, hit buffer and counters; the walk that classifies the
    visits is the oracle's (xl_classes asserts its visits and descents, and its
    frame, against the C oracle); the recorded counts are the classifier's; and
    every class the case is in the table for has at least 8 visits.  The cases
    with exact zeros are anchored at GRID_FRAMES' other frames too."""
    e, xf, classes, _ = S.XL_CASES[name]
    sc = S.xl_grid(e)
    _anchor(sc, 0, xf, what=f"xl {name}")
    got = S.xl_classes(sc, xf)
    print(name, dict(zip(S.XL_CLASSES, got)))
    assert got == S.XL_COUNTS[name], (name, got)
    for c in classes:
        assert got[S.XL_CLASSES.index(c)] >= 8, (name, c, got)
    assert (xf.reshape(3, 4)[:, 3] != 0).any()           # an offset: the translated walk
    if name in S.XL_ALL_FRAMES:
        for w, h in S.GRID_FRAMES[1:]:
            _anchor(S.xl_grid(e, w, h), 0, xf, what=f"xl {name} {w}x{h}")
            _anchor(S.xl_grid(e, w, h), 0, xf, shadow=True, what=f"xl {name} {w}x{h} shadow")
    _anchor(sc, 0, xf, shadow=True, what=f"xl {name} shadow")


def test_xl_table_reaches_every_class():
    """Over the table every class of XL_CLASSES is reached by a case that is
    listed for it: all four combinations of lt / gt with s == -1 / s == +1
    among them; each by a case that proves the translated float walk
    (RT_OPT_FAST_USED & 4, asserted on the GPU), and each by a case with a
    rotation too, but the guard's far side (guard+-, below+-, tiny-), which
    the rotation does not change."""
    assert set(S.XL_COUNTS) == set(S.XL_CASES)
    listed = {c: [n for n, case in S.XL_CASES.items() if c in case[2]] for c in S.XL_CLASSES}
    for c, names in listed.items():
        assert names, c
        assert any(S.XL_CASES[n][3] for n in names), c
        assert all(S.XL_COUNTS[n][S.XL_CLASSES.index(c)] >= 8 for n in names), c
        if c not in ("guard+", "guard-", "below+", "below-", "tiny-"):
            assert any((S.XL_CASES[n][1].reshape(3, 4)[:, :3] != np.eye(3, dtype=F)).any() for n in names), c
    assert {"lt_-1", "gt_-1", "lt_+1", "gt_+1"} <= set(listed)
    # the one offset the suite had before reaches none of the tie or tiny classes
    old = S.xl_classes(S.xl_grid(0), S.rot_y(0.0, (0.01, -0.005, 0.02)))
    assert [old[S.XL_CLASSES.index(c)] for c in ("s0x", "s0y", "s0z", "tiny+", "tiny-", "guard+", "guard-", "lt_eq<1",
                                                     "lt_eq>1")] == [0] * 9


class _NumpyKernel:
    """A numpy restatement of a kernel in the place of a SynthScene's live
    camera: render() as test_gpu_synth._kd calls it."""

    def __init__(self, sc, form):
        self.sc, self.form, self.out = sc, form, {}

    def render(self, mode, xform=None, count=False, shadow=False):
        assert mode == 0 and not shadow
        if not self.out:
            self.out[0] = S.xl_render(self.sc, xform, self.form)
        argb, hit, cnt = self.out[0]
        return argb, hit, cnt if count else None


def test_xl_float_forms_pass_the_comparison():
    """xfast_slot's forms restated (lt_eps_x / gt_eps_x, the double forms for
    |s| < 2^-20, s1 in double) give the oracle's frame, hit buffer and counters
    on every case: the comparison of the GPU tests passes them."""
    from tests.test_gpu_synth import _kd
    for name, (e, xf, _, _) in S.XL_CASES.items():
        sc = S.xl_grid(e)
        _kd(_NumpyKernel(sc, "float"), sc.oracle(0, xform=xf), 3, xf, what=f"xl {name} float forms")


@pytest.mark.parametrize("fault", S.XL_FAULTS)
def test_xl_a_wrong_kernel_fails_the_comparison(fault):
    """Five plausible wrong kernels (XL_FAULTS) restated in numpy and fed to
    the comparison the GPU tests use (test_gpu_synth._kd, as kernel 3): each
    fails it on the case XL_CATCHES names, on which the faultless float forms
    pass.  (a) is caught by the case with a rotation of 2^-60 alone: a tiny
    lane's float compare differs from the double form only where maxt0 * dir
    or mint1 * dir lies within 1e-16 of s without being equal to it, which
    takes a ray component below 2^-33; the frames without that rotation have
    exact zeros there, and 0 == s is decided alike by both."""
    from tests.test_gpu_synth import _kd
    name = S.XL_CATCHES[fault]
    e, xf, _, _ = S.XL_CASES[name]
    sc = S.xl_grid(e)
    want = sc.oracle(0, xform=xf)
    _kd(_NumpyKernel(sc, "float"), want, 3, xf, what=f"xl {name} float forms")
    with pytest.raises(AssertionError):
        _kd(_NumpyKernel(sc, fault), want, 3, xf, what=f"xl {name} {fault}")
