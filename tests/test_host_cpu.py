"""CPU tests: the C ABI library's host half, the oracle against its pins
(golden fixtures from the independent numpy restatement, hand-derived
known answers), and the sharding logic.  No GPU calls."""
import hashlib
import os
import re

import numpy as np
import pytest

from cpp_cuda_raytracer_dev_amd import _lib, raytracer as R, scenes
from oracle import _oracle as O, np_oracle as N
from tests import helpers as H

PLY_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ply")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_mi355x.h")


def test_library_exports_every_declared_symbol():
    decl = set(re.findall(r"\b(rt_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    L = _lib.lib()
    missing = [s for s in sorted(decl) if not hasattr(L, s)]
    assert not missing, missing
    assert decl == set(_lib.SIGNATURES), set(_lib.SIGNATURES) ^ decl
    assert L.rt_abi_version() == 2


def test_cpp_facade_and_headless_driver_compile(tmp_path):
    """The reference-shaped C++ facade (include/rt_facade.hpp) and the
    WinMain replacement build against the C ABI."""
    import subprocess
    root = os.path.dirname(HEADER)
    src = os.path.join(os.path.dirname(root), "tools", "rt_headless.cpp")
    out = tmp_path / "rt_headless"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", root, "-o", str(out), src, _lib.LIB_PATH],
                   check=True)
    assert out.exists()


def test_ctypes_structs_match_header(tmp_path):
    """The Python mirrors of the ABI's structs have the C layout (size and
    every field's offset), compiled from include/rt_mi355x.h here."""
    import ctypes as C
    import subprocess
    structs = {"rt_frame_loop": _lib.RtFrameLoop, "rt_tile": _lib.RtTile}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rt_mi355x.h"', "int main(void) {"]
    for name, py in structs.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for f in py._fields_:
            lines.append(f'printf("{name} {f[0]} %zu\\n", offsetof({name}, {f[0]}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for line in filter(None, got):
        name, field, val = line.split()
        py = structs[name]
        want = C.sizeof(py) if field == "size" else getattr(py, field).offset
        assert int(val) == want, (name, field, int(val), want)


def test_epsilon_threshold_is_exact():
    c = np.array([0x24E69595], np.uint32).view(np.float32)[0]
    assert np.float64(c) >= 1e-16
    assert np.float64(np.nextafter(c, np.float32(0))) < 1e-16
    assert np.float64(1) + 1e-16 == 1.0  # (u+v) > 1 + 1e-16  <=>  (u+v) > 1.0f


@pytest.mark.parametrize("name", list(scenes.FIXTURE_MODES))
def test_mesh_assembly_matches_oracle(name):
    v, a, ix = scenes.fixture_mesh(name)
    pts, n, leafs = R.assemble_mesh(v, H.faces_list(a, ix))
    opts, oleafs = O.assemble(v, a, ix)
    assert pts.tobytes() == opts.tobytes()
    for f in ("x0", "x1", "y0", "y1", "z0", "z1"):
        assert leafs[f].tobytes() == oleafs[f].tobytes()
    assert (leafs["tri"] == np.arange(n)).all()


def _ply_file(name, tmp_path):
    """Path of the reference's own <name>.ply (tests/golden/ply/: the file as
    it ships, rabbit_70k.ply xz-compressed and unpacked into tmp_path)."""
    path = os.path.join(PLY_DIR, name + ".ply")
    if os.path.exists(path):
        return path
    import lzma
    out = tmp_path / (name + ".ply")
    with lzma.open(path + ".xz") as fp:
        out.write_bytes(fp.read())
    return str(out)


@pytest.mark.parametrize("name,mode", list(scenes.FIXTURE_MODES.items()))
def test_ply_loader_matches_oracle_and_fixture(name, mode, tmp_path):
    path = _ply_file(name, tmp_path)
    pts, n, leafs = R.read_ply(path, mode)
    opts, oleafs = O.read_ply(path, mode)
    v, a, ix = scenes.fixture_mesh(name)
    fpts, _, _ = R.assemble_mesh(v, H.faces_list(a, ix))
    assert pts.tobytes() == opts.tobytes() == fpts.tobytes()


def test_ply_loader_errors(tmp_path):
    p = tmp_path / "bad.ply"
    p.write_text("ply\nformat ascii 1.0\nelement vertex 3\nelement face 1\nend_header\n0 0 0\n1 0 0\n0 1 0\n5 0 1 2 0 1\n")
    with pytest.raises(_lib.RtError):
        R.read_ply(str(p), 0)
    with pytest.raises(_lib.RtError):
        R.read_ply(str(tmp_path / "missing.ply"), 0)
    q = tmp_path / "ok.ply"
    scenes.write_ply(str(q), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32),
                     np.array([[0, 1, 2], [1, 3, 2]], np.int32))
    pts, n, _ = R.read_ply(str(q), 0)
    assert n == 2 and pts[0, :3].tolist() == [0, 1, 0]  # 3-gon stored (P3, P1, P2)


def _nodes_equal(a, b):
    for f in ("cut_flag", "is_leaf", "tri_index", "left", "right", "parent"):
        assert (a[f] == b[f]).all(), f
    for f in ("x0", "x1", "y0", "y1", "z0", "z1"):
        assert a[f].tobytes() == b[f].tobytes(), f
    inner = a["is_leaf"] == 0
    for f in ("s1", "s2"):
        assert a[f][inner].tobytes() == b[f][inner].tobytes(), f


@pytest.mark.parametrize("name", list(scenes.FIXTURE_MODES))
def test_kd_build_matches_oracle(name):
    pn, on = H.trees(name)
    _nodes_equal(pn, on)


def _random_leafs(n, seed, ties):
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 8, size=(n, 3)).astype(np.float32) if ties else rng.random((n, 3)).astype(np.float32)
    hi = lo + (rng.integers(0, 3, size=(n, 3)).astype(np.float32) if ties else rng.random((n, 3)).astype(np.float32))
    pl = np.zeros(n, _lib.LEAF_AABB_DTYPE)
    ol = np.zeros(n, O.LEAF_DTYPE)
    for i, f in enumerate(("x", "y", "z")):
        for arr in (pl, ol):
            arr[f + "0"] = lo[:, i]
            arr[f + "1"] = hi[:, i]
    pl["tri"] = np.arange(n)
    ol["tri"] = np.arange(n)
    return pl, ol


@pytest.mark.parametrize("n,seed,ties", [(1, 0, False), (2, 1, False), (3, 2, True), (17, 3, True),
                                         (1000, 4, True), (4097, 5, False), (30000, 6, True)])
def test_kd_build_random_with_ties(n, seed, ties):
    pl, ol = _random_leafs(n, seed, ties)
    _nodes_equal(R.kd_build(pl, nthreads=4), O.build_kd(ol))


def test_kd_invariants():
    pts, leafs, _ = H.mesh("rabbit_70k")
    nodes = H.trees("rabbit_70k")[0]
    n = len(leafs)
    assert len(nodes) == 2 * n - 1
    leaf = nodes["is_leaf"] == 1
    assert sorted(nodes["tri_index"][leaf]) == list(range(n))
    inner = np.flatnonzero(~leaf)
    assert (nodes["right"][inner] == nodes["left"][inner] + 1).all()
    assert (nodes["left"][inner] > inner).all()
    for side in ("left", "right"):
        c = nodes[side][inner]
        for f in ("x0", "y0", "z0"):
            assert (nodes[f][c] >= nodes[f][inner]).all()
        for f in ("x1", "y1", "z1"):
            assert (nodes[f][c] <= nodes[f][inner]).all()
    depth = np.zeros(len(nodes), int)
    for i in inner:
        depth[nodes["left"][i]] = depth[nodes["right"][i]] = depth[i] + 1
    assert depth.max() + 1 <= int(np.ceil(np.log2(2 * n - 1)))  # the reference's stack size suffices


@pytest.mark.parametrize("w,h", [(320, 180), (960, 540), (1920, 1080), (3840, 2160), (81, 45), (1, 1)])
def test_camera_basis_matches_oracle(w, h):
    c = O.camera(w, h)
    b = R.camera_basis(w, h, R.film_w(w, h), np.float32(.024), np.float32(.055), (0, .1, -1), (0, .1, 0), (0, 1, 0))
    for k in ("n", "u", "v", "n_mod", "u_mod", "v_mod"):
        assert np.array(getattr(c, k)[:], np.float32).tobytes() == b[k].tobytes(), k
    nb = N.camera(w, h)
    for k in ("n_mod", "u_mod", "v_mod"):
        assert np.array(nb[k], np.float32).tobytes() == b[k].tobytes(), k


def test_fast_rsqrt_against_numpy_restatement():
    rng = np.random.default_rng(0)
    for s in rng.random(200).astype(np.float32) * 10:
        a = np.float32(O.lib().orc_device_inverse_sqrt(s, 0.0, 0.0))
        b = N.rsqrt(np.float32(s * s), 21)
        assert a.tobytes() == b.tobytes()
        c = np.float32(O.lib().orc_host_vector_norm(s))
        assert c.tobytes() == N.rsqrt(s, 8).tobytes()


# ---------------------------------------------------------------- oracle pins

@pytest.mark.parametrize("name,w,h", [("dump_test", 64, 36), ("tester", 80, 45), ("dump", 48, 27)])
@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_matches_numpy_golden(name, w, h, mode):
    g = H.golden()
    argb, hit, _ = H.oracle_render(name, w, h, mode)
    key = f"{name}_{w}x{h}_m{mode}"
    assert (hit == g[key + "_hit"]).all()
    assert (argb == g[key + "_argb"]).all()


@pytest.mark.parametrize("key,name,w,h,mode", [("tester_320x180_m0", "tester", 320, 180, 0),
                                               ("tester_320x180_m1", "tester", 320, 180, 1),
                                               ("rabbit_70k_960x540_m0", "rabbit_70k", 960, 540, 0),
                                               ("dump_320x180_m0", "dump", 320, 180, 0)])
def test_oracle_matches_recorded_hashes(key, name, w, h, mode):
    g = H.golden()
    argb, hit, cnt = H.oracle_render(name, w, h, mode)
    assert hashlib.sha256(argb.tobytes()).hexdigest() == str(g[key + "_argb_sha"])
    assert hashlib.sha256(hit.tobytes()).hexdigest() == str(g[key + "_hit_sha"])
    assert (cnt == g[key + "_counters"]).all()


@pytest.mark.parametrize("key", ["tester_320x180_m0", "tester_320x180_m1", "rabbit_70k_960x540_m0",
                                 "rabbit_70k_1920x1080_m0_fill"])
def test_oracle_reproduces_frame_hashes(key):
    """The committed full-frame hashes the GPU tests and bench.py check
    (tests/golden/frame_hashes.json) are the oracle's own frames: the cheap
    ones are re-rendered here (the rest take the oracle minutes, or the
    stand-in KD build)."""
    ent = H.frame_hashes()[key]
    assert H.mesh_matches(ent)
    argb, hit, cnt = H.oracle_render(ent["scene"], ent["w"], ent["h"], ent["mode"], cam_kw=H.view_kw(ent),
                                     shadow=ent["shadow"])
    assert hashlib.sha256(argb.tobytes()).hexdigest() == ent["argb_sha"]
    assert hashlib.sha256(hit.tobytes()).hexdigest() == ent["hit_sha"]
    assert [int(x) for x in cnt] == ent["counters"]


def test_frame_hash_views_cover_90_percent():
    """README.md:19 quotes ~25 FPS at "90%+ pixel coverage": the fill views'
    recorded coverage is >= 0.9 at every resolution."""
    fill = [e for e in H.frame_hashes().values() if e["view"] == "fill"]
    assert len(fill) >= 3
    for e in fill:
        assert e["coverage"] >= 0.9, e


def test_numpy_crosscheck_with_transform():
    """The two restatements agree on a non-identity object transform (rotated + translated)."""
    v, a, ix = scenes.fixture_mesh("dump")
    pts, boxes = N.assemble(v, a, ix)
    nodes = N.build_kd(boxes)
    ang = np.deg2rad(12.0)
    c, s = np.float32(np.cos(ang)), np.float32(np.sin(ang))
    X = np.array([c, 0, s, 0.004, 0, 1, 0, -0.002, -s, 0, c, 0.01], np.float32)
    cam = N.camera(40, 24)
    argb, hit = N.render(pts, nodes, cam, 0, xform=X)
    oargb, ohit, _ = H.oracle_render("dump", 40, 24, 0, xform=X)
    assert (hit >= 0).sum() > 5
    assert (hit == ohit).all() and (argb == oargb).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_known_answer_dump_test(mode):
    """Hand-derived KAT on dump_test.ply: seven coplanar z=0 triangles, four of
    them copies of {0,3,4} with permuted windings.  Every primary ray meets
    the plane; a pixel must hit one of the triangles that contain its plane
    point, and where exactly one triangle contains it (away from edges), that
    triangle."""
    w, h = 64, 36
    argb, hit, _ = H.oracle_render("dump_test", w, h, mode)
    v, a, ix = scenes.fixture_mesh("dump_test")
    faces = np.asarray(ix).reshape(-1, 3)
    assert (hit >= 0).all()
    cam = O.camera(w, h)
    P = v.astype(np.float64)

    def side(u, v_, p):
        return (v_[0] - u[0]) * (p[1] - u[1]) - (v_[1] - u[1]) * (p[0] - u[0])

    def inside(p, tri, margin):
        A, B, C = (P[i, :2] for i in tri)
        d = np.array([side(A, B, p), side(B, C, p), side(C, A, p)])
        return bool((d > margin).all() or (d < -margin).all())

    unique = 0
    for iy in range(h):
        for ix_ in range(w):
            r = np.zeros(3, np.float32)
            O.lib().orc_primary_ray(cam, ix_, iy, r.ctypes.data)
            t = 1.0 / r[2]
            p = np.array([t * r[0], 0.1 + t * r[1]])
            loose = [k for k, f in enumerate(faces) if inside(p, f, -1e-3)]
            tight = [k for k, f in enumerate(faces) if inside(p, f, 1e-3)]
            got = hit[iy * w + ix_]
            assert got in loose, (ix_, iy, got, loose)
            if len(loose) == 1 and len(tight) == 1:
                assert got == tight[0]
                unique += 1
    assert unique > 500


def test_single_triangle_analytic_distance():
    """One triangle facing the camera: the hit distance is the analytic t."""
    verts = np.array([[-4, -4, 0.5], [4, -4, 0.5], [0, 4, 0.5]], np.float32)
    pts, n, leafs = R.assemble_mesh(verts, np.array([[0, 1, 2]], np.int32))
    nodes = R.kd_build(leafs)
    on = O.build_kd(O.assemble(verts, np.array([3], np.int32), np.array([0, 1, 2], np.int32))[1])
    cam = O.camera(9, 5)
    s = O.Scene(pts, O.default_rad(1), on, cam)
    argb, hit, cnt = s.render(0)
    assert (hit == 0).all() and len(nodes) == 1
    assert (argb != R.BACKGROUND_ARGB).all()
    # centre pixel: ray through (0, 0.1) direction ~ +z, distance ~ 1.5
    r = np.zeros(3, np.float32)
    O.lib().orc_primary_ray(cam, 4, 2, r.ctypes.data)
    assert abs(1.5 / r[2] - 1.5) < 1e-3


# ---------------------------------------------------------------- shadow rays

@pytest.mark.parametrize("name,w,h", [("dump", 40, 24), ("rabbit_70k", 64, 36)])
def test_shadow_oracle_matches_numpy_golden(name, w, h):
    """RT_FLAG_SHADOW: the C oracle against the numpy restatement's frames."""
    g = H.golden()
    argb, hit, _ = H.oracle_render(name, w, h, 0, shadow=True)
    key = f"{name}_{w}x{h}_shadow"
    assert (hit == g[key + "_hit"]).all()
    assert (argb == g[key + "_argb"]).all()
    assert ((argb == 0) & (hit >= 0)).sum() > 10


@pytest.mark.parametrize("name,w,h", [("rabbit_70k", 960, 540), ("dump", 320, 180)])
def test_shadow_oracle_matches_recorded_hashes(name, w, h):
    g = H.golden()
    argb, hit, cnt = H.oracle_render(name, w, h, 0, shadow=True)
    key = f"{name}_{w}x{h}_shadow"
    assert hashlib.sha256(argb.tobytes()).hexdigest() == str(g[key + "_argb_sha"])
    assert (cnt == g[key + "_counters"]).all()


@pytest.mark.parametrize("name,w,h", [("dump", 40, 24), ("rabbit_70k", 64, 36), ("tester", 48, 27)])
def test_shadow_segment_walk_same_images(name, w, h):
    """Round 6: the shadow walk enters a box only below Lmax (oracle.c
    trace_shadow).  The numpy restatement walking the whole ray beyond the
    hit, as rounds 1-5 defined it, gives the same images, and the segment walk
    the committed golden ones."""
    from cpp_cuda_raytracer_dev_amd import scenes
    from oracle import np_oracle as N
    v, a, ix = scenes.fixture_mesh(name)
    pts, boxes = N.assemble(v, a, ix)
    nodes, cam = N.build_kd(boxes), N.camera(w, h)
    seg, seg_hit = N.render(pts, nodes, cam, 0, shadow=True)
    ray, ray_hit = N.render(pts, nodes, cam, 0, shadow=True, segment=False)
    assert (seg_hit == ray_hit).all() and (seg == ray).all()
    g = H.golden()
    key = f"{name}_{w}x{h}_shadow"
    if key + "_argb" in g.files:
        assert (seg == g[key + "_argb"]).all()


def test_shadow_only_darkens_hit_pixels():
    """Shadows change nothing but the colour of some hit pixels (to 0), and
    add the shadow walks' visits to the counters."""
    a0, h0, c0 = H.oracle_render("rabbit_70k", 320, 180, 0)
    a1, h1, c1 = H.oracle_render("rabbit_70k", 320, 180, 0, shadow=True)
    assert (h0 == h1).all()
    changed = a0 != a1
    assert (h0[changed] >= 0).all() and (a1[changed] == 0).all()
    assert 0 < changed.sum() < (h0 >= 0).sum()
    assert c1[3] == c0[3] and c1[0] > c0[0] and c1[1] > c0[1]


def test_shadow_matches_bruteforce_segment_test():
    """Geometric meaning of the shadow definition: the KD walk from the light
    finds an occluder on the light->hit segment for (almost) exactly the
    pixels a float64 brute-force test over every triangle does (the rest are
    epsilon/boundary cases of the reference's traversal rules)."""
    import ctypes as C
    name, w, h = "rabbit_70k", 160, 90
    pts, _, _ = H.mesh(name)
    a0, hit, _ = H.oracle_render(name, w, h, 0)
    a1, _, _ = H.oracle_render(name, w, h, 0, shadow=True)
    cam = O.camera(w, h)
    pos = np.array(cam.pos[:3], np.float64)
    T = pts.reshape(-1, 3, 3).astype(np.float64) - pos
    p0, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]

    def mt(o, dv):
        pv = np.cross(dv, e2)
        det = (pv * e1).sum(1)
        with np.errstate(all="ignore"):
            inv = 1 / det
            tv = o - p0
            u = (tv * pv).sum(1) * inv
            q = np.cross(tv, e1)
            return u, (q * dv).sum(1) * inv, (q * e2).sum(1) * inv, np.abs(det) > 1e-20

    idx = np.flatnonzero(hit >= 0)
    out = (C.c_float * 3)()
    agree = 0
    for i in idx:
        iy, ix = divmod(int(i), w)
        O.lib().orc_primary_ray(C.byref(cam), ix, iy, out)
        r = np.array(out[:], np.float64)
        k = hit[i]
        t_hit = mt(np.zeros(3), r)[2][k]
        seg = t_hit * r - 2.0
        L = np.linalg.norm(seg)
        u, v, t, ok = mt(np.full(3, 2.0), seg / L)
        occ = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-12) & (t < 0.999 * L)
        occ[k] = False
        agree += bool(occ.any()) == bool(a1[i] == 0)
    assert len(idx) > 400 and agree >= 0.99 * len(idx)


# ---------------------------------------------------------------- sharding

def test_band_pack_unpack_roundtrip():
    from cpp_cuda_raytracer_dev_amd import distributed as D
    rng = np.random.default_rng(1)
    for (w, h) in [(1920, 1080), (33, 17), (8, 8), (5, 3)]:
        frame = rng.integers(0, 2**32, size=w * h, dtype=np.uint64).astype(np.uint32)
        for n in (1, 2, 3, 8):
            g = np.concatenate([D.pack_bands_numpy(frame, w, h, n, r) for r in range(n)])
            assert D.packed_pixels(w, h, n) == R.packed_pixels(w, h, n)
            assert (D.unpack_bands_numpy(g, w, h, n) == frame).all()


def test_knot_standin_is_closed_manifold():
    """The torus-knot stand-in (scenes.STANDINS["knot"]): the dragon's
    triangle count inside the dragon's box, every edge shared by exactly two
    triangles (a closed 2-manifold, like the blob stand-ins), deterministic."""
    v, f = scenes.standin("knot")
    assert len(f) == 871_414 and np.isfinite(v).all()
    lo, hi = np.array(scenes.STANDINS["knot"][1]), np.array(scenes.STANDINS["knot"][2])
    assert np.allclose(v.min(0), lo, atol=1e-6) and np.allclose(v.max(0), hi, atol=1e-6)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1).astype(np.int64)
    _, cnt = np.unique(e[:, 0] * len(v) + e[:, 1], return_counts=True)
    assert (cnt == 2).all()
    v2, f2 = scenes.standin("knot")
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes()
    assert scenes.mesh_sha("knot") == H.frame_hashes()["knot_1920x1080_m0"]["mesh_sha"]
