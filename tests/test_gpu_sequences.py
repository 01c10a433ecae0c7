"""Random sequences of options, trees, targets and frame loops on cameras and
scenes that stay alive (tests/seq.py): every render of every sequence is the
stateless oracle's frame, hit index, counters and planes, bit for bit.  What
the sequences hold is proved on the CPU (tests/test_seq_cpu.py).  A failure's
message carries the seed, the step and the operations up to it as a literal
for ``tests.seq.replay``; the shortest failing sequence found goes into
tests/golden/sequences.json, which test_recorded replays."""
import json
import os
import time

import numpy as np
import pytest

from tests import seq as Q

pytestmark = pytest.mark.gpu

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequences.json")


@pytest.fixture(scope="module")
def oracle():
    o = Q.Oracle()
    yield o
    o.close()


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_sequence(oracle, seed):
    ops = Q.generate(seed)
    t0 = time.perf_counter()
    r = Q.replay(ops, seed=seed, oracle=oracle)
    print(f"seed {seed}: {len(ops)} operations, {r.renders} compared renders and loops "
          f"({r.passes} deferred shadow passes among them), {time.perf_counter() - t0:.2f} s")
    assert len(r.done) == len(ops) and r.renders >= 60


def test_recorded(oracle):
    """The sequences that once failed (a list of operation lists; data only)."""
    with open(RECORDED) as fp:
        recorded = json.load(fp)
    assert isinstance(recorded, list)
    for k, ops in enumerate(recorded):
        r = Q.replay(ops, seed=f"recorded {k}", oracle=oracle)
        assert len(r.done) == len(ops)


def test_debug_statistics_start_from_zero():
    """RT_OPT_DEBUG with bit 16384 (record-load statistics) zeroes the 32
    counters it shares with the per-wave stamps of bit 2: after a bit-2 render
    the first 32 words read as they do on a fresh camera given the same 16384
    render (zeros, in a build whose kernels do not write the statistics),
    not the stamps' start clocks."""
    from cpp_cuda_raytracer_dev_amd import _lib, raytracer as R
    w = Q.world()
    wd, ht = Q.CAMS[0]
    trixel = R.Trixel(Q.NTRI["s257"], w.pts["s257"])
    trixel.set_kd_nodes(w.trees["s257"]["built"])
    cams, objs = [], []
    try:
        reads = []
        for stamps_first in (True, False):
            cam = R.Camera.default(wd, ht)
            cams.append(cam)
            obj = R.Object(trixel)
            objs.append(obj)
            cam.add_object(obj)
            if stamps_first:
                cam.set_option(_lib.RT_OPT_DEBUG, 2)
                obj.render(cam)
                stamps = np.zeros(32, np.uint64)
                assert _lib.lib().rt_camera_debug_read(cam._h, _lib.ptr(stamps), 32) == 32
                assert stamps.any(), "the bit-2 render left no stamps: the test would see nothing"
            cam.set_option(_lib.RT_OPT_DEBUG, 16384)
            obj.render(cam, flags=R.RT_FLAG_WRITE_HIT)
            cam.color_pixels()
            out = np.full(32, 0xAB, np.uint64)
            assert _lib.lib().rt_camera_debug_read(cam._h, _lib.ptr(out), 32) == 32
            reads.append(out)
            assert cam.device_error() == 0
        assert (reads[0] == reads[1]).all(), (reads[0], reads[1])
    finally:
        for cam in cams:
            cam.close()
        for obj in objs:
            if obj.motion is not None:
                obj.motion.close()
        trixel.close()
