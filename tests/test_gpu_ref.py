"""The HIP kernels against the reference's own code, with no oracle in between.

oracle/_ref/libref.so is the reference's sources compiled for the CPU
(oracle/ref_build.py; tests/test_ref_cpu.py pins the oracle with it).  Here a
dozen of the smallest scenes of that module go through the product's kernels
and through the reference's intersect_voxel_cuda / intersect_trixel_cuda and
color_cam_cuda, and the hit index, the ARGB frame and the ten planes of
RT_FLAG_WRITE_AOV are compared bit for bit: if the oracle and the kernels
were wrong together, this would still move.

Only what build() left in oracle/_ref/ is used: the reference tree is not
read.  On a host that has neither (a clean checkout on a GPU machine: the
reference is not there to compile) the module skips, with that reason.
"""
import functools

import numpy as np
import pytest

from oracle import _oracle as O, _ref as Rf
from tests import synth as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not Rf.available(), reason=Rf.why_missing())]

F = np.float32
W, H = 32, 18


def _tree(name):
    (v, f), trees = S.tree_variants()
    return dict(verts=v, faces=f, nodes=trees[name])


def _mesh(vf):
    return dict(verts=vf[0], faces=vf[1])


#: name -> (SynthScene arguments, object transform, modes); the transformed cases are KD only
#: (the flat kernel reads no transform)
CASES = {
    "soup33": (dict(**_mesh(S.soup(33, S.SOUP_SEED + 33)), w=W, h=H), None, (0, 1)),
    "edge_soup12": (dict(**_mesh(S.edge_soup(12, S.EDGE_SEED + 12)), w=W, h=H), None, (0, 1)),
    "grid": (dict(**_mesh(S.grid()), w=S.W, h=S.H_), None, (0, 1)),           # zero components, zero bounds
    "copies": (dict(**_mesh(S.copies(*S.COPIES)), w=W, h=H), None, (0, 1)),   # exact depth ties
    "threshold_below": (dict(**_mesh(S.threshold_triangle(-1, False, True)), w=S.W, h=S.H_, cam_kw=S.THRESHOLD_CAM),
                        None, (0, 1)),
    "threshold_at": (dict(**_mesh(S.threshold_triangle(0, False, True)), w=S.W, h=S.H_, cam_kw=S.THRESHOLD_CAM),
                     None, (0, 1)),
    "tree_inflated_split": (lambda: dict(**_tree("inflated_split"), w=S.W, h=S.H_), None, (0,)),
    "materials": (dict(**_mesh(S.soup(S.LIGHT_N, S.SOUP_SEED + S.LIGHT_N)), w=W, h=H,
                       rad=S.material_table("materials", S.LIGHT_N)), None, (0, 1)),
    "soup33_rot": (dict(**_mesh(S.soup(33, S.SOUP_SEED + 33)), w=W, h=H), S.rot_y(17.0), (0,)),
    "soup33_xlate": (dict(**_mesh(S.soup(33, S.SOUP_SEED + 33)), w=W, h=H), S.rot_y(0.0, (0.01, -0.005, 0.02)), (0,)),
}
KD_CONFIGS = [dict(kernel=2), dict(kernel=3, rays=8), dict(kernel=3, rays=16), dict(kernel=3, rays=32)]
FLAT_CONFIGS = [dict(flat=9), dict(flat=12)]
RUNS = [(name, mode, cfg) for name, (_, _, modes) in CASES.items() for mode in modes
        for cfg in (KD_CONFIGS if mode == 0 else FLAT_CONFIGS)]


def _scene(name, **opts):
    kw = CASES[name][0]
    kw = dict(kw() if callable(kw) else kw)
    return S.SynthScene(kw.pop("verts"), kw.pop("faces"), kw.pop("w"), kw.pop("h"), **kw, **opts)


@functools.lru_cache(None)
def reference_frame(name, mode):
    """The first frame of a fresh reference scene: (hit, planes [10, n], argb
    after the SET pass: background + Phong)."""
    sc = _scene(name)
    rad = O.default_rad(len(sc.pts)) if sc.rad is None else sc.rad
    with Rf.Scene(sc.w, sc.h, sc.pts, rad, nodes=sc.onodes, **sc.okw) as rsc:
        rsc.set_xform(CASES[name][1])
        hit, aov, _, clean = rsc.frame(mode)
    for a in (hit, aov, clean):
        a.setflags(write=False)
    return hit, aov, clean


@pytest.mark.parametrize("name,mode,cfg", RUNS,
                         ids=[f"{n}-m{m}-" + "-".join(f"{k}{v}" for k, v in c.items()) for n, m, c in RUNS])
def test_kernels_equal_the_reference(name, mode, cfg):
    rhit, raov, rargb = reference_frame(name, mode)
    assert (rhit >= 0).any() or name == "threshold_below"
    with _scene(name, **cfg) as sc:
        argb, hit, _ = sc.render(mode, xform=CASES[name][1], aov=True)
        a = sc.cam.aov()
        assert sc.cam.device_error() == 0
        n = sc.w * sc.h
    planes = np.concatenate([a["d"].reshape(1, n), a["pnt"].reshape(3, n), a["norm"].reshape(3, n),
                             a["rad"].reshape(3, n)]).view(np.uint32)
    bad = np.flatnonzero(hit != rhit)
    assert bad.size == 0, ("hit", bad.size, bad[:6], hit[bad[:6]], rhit[bad[:6]])
    bad = np.flatnonzero(argb != rargb)
    assert bad.size == 0, ("argb", bad.size, bad[:6], argb[bad[:6]], rargb[bad[:6]])
    want = raov.view(np.uint32)
    bad = np.flatnonzero((planes != want).any(0))
    assert bad.size == 0, ("planes", bad.size, bad[:6], planes[:, bad[:2]], want[:, bad[:2]])
