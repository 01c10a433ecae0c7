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
