"""GPU KD builder (rt_kd_build_gpu / rt_scene_build_kd)
against the host builder rt_kd_build, which tests/test_host_cpu.py proves
equal to the literal restatement of Trixel::create_kd (TD/Trixel.h:135-473)
and merge_sort (TD/sort.h:11-60).  Byte-for-byte on the whole node array."""
import hashlib

import numpy as np
import pytest

from cpp_cuda_raytracer_dev_amd import _lib, raytracer as R, scenes
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _same_nodes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if a.tobytes() != b.tobytes():
        ab = a.view(np.uint8).reshape(len(a), -1)
        bb = b.view(np.uint8).reshape(len(b), -1)
        bad = np.flatnonzero((ab != bb).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} nodes differ, first {bad[:5]}: {a[bad[:2]]} vs {b[bad[:2]]}")


@pytest.mark.parametrize("name", list(scenes.FIXTURE_MODES) + ["dragon", "happy", "big"])
def test_gpu_build_equals_host_build(name):
    leafs = H.mesh(name)[1]
    _same_nodes(R.kd_build_gpu(leafs), H.product_tree(name), name)


_random_leafs = H.random_leafs  # (shared with tests/test_ref_cpu.py)


@pytest.mark.parametrize("n,seed,ties,zeros", [(1, 0, False, False), (2, 1, False, False), (3, 2, True, False),
                                               (7, 3, True, True), (17, 4, True, False), (1000, 5, True, True),
                                               (4097, 6, False, False), (65537, 7, True, True),
                                               (300001, 8, False, True)])
def test_gpu_build_random_ties(n, seed, ties, zeros):
    pl = _random_leafs(n, seed, ties, zeros)
    _same_nodes(R.kd_build_gpu(pl), R.kd_build(pl, nthreads=4), f"random n={n}")


def test_gpu_build_rejects_bad_input():
    pl = _random_leafs(10, 0, False)
    pl["tri"][3] = pl["tri"][4]
    with pytest.raises(_lib.RtError):
        R.kd_build_gpu(pl)
    pl = _random_leafs(10, 0, False)
    pl["x0"][2] = np.nan
    with pytest.raises(_lib.RtError):
        R.kd_build_gpu(pl)


@pytest.mark.parametrize("name,key", [("dragon", "dragon_960x540_m0"), ("rabbit_70k", "rabbit_70k_960x540_m0")])
def test_scene_built_on_device_renders_oracle_frame(name, key):
    """Trixel.create_kd(on_device=True): the tree is built where it is used
    (rt_scene_build_kd) and the frame is the oracle's (committed hash)."""
    ent = H.frame_hashes()[key]
    pts, leafs, _ = H.mesh(name)
    t = R.Trixel(len(pts), pts)
    t.set_sorted_voxels(leafs, len(leafs))
    assert t.create_kd(on_device=True) == 0
    _same_nodes(t.read_kd_nodes(), H.product_tree(name), name)
    cam = R.Camera.default(ent["w"], ent["h"])
    obj = R.Object(t)
    cam.add_object(obj)
    obj.render(cam, flags=R.RT_FLAG_WRITE_HIT)
    cam.color_pixels()
    if H.mesh_matches(ent):
        assert hashlib.sha256(cam.h_color.tobytes()).hexdigest() == ent["argb_sha"]
        assert hashlib.sha256(cam.h_rmi.tobytes()).hexdigest() == ent["hit_sha"]
