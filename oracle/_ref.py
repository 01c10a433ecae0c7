"""ctypes binding of oracle/_ref/libref.so: the reference's own sources compiled
for the CPU (oracle/ref_build.py) behind the C ABI of oracle/ref_harness.cpp.

TEST INFRASTRUCTURE ONLY: imported by tests/test_ref_cpu.py and
tests/test_gpu_ref.py.  The product package, smoke() and bench.py never load
it.  Arrays use the oracle binding's dtypes (oracle/_oracle.py): the harness
copies the reference's structures into LEAF_DTYPE / NODE_DTYPE / OrcCamera.
"""
from __future__ import annotations

import ctypes as C
import os
import struct

import numpy as np

from . import ref_build
from ._oracle import LEAF_DTYPE, NODE_DTYPE, OrcCamera

LIB_PATH = ref_build.LIB_PATH
ASAN_PATH = ref_build.ASAN_PATH
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)

_lib = None


def build():
    """oracle/ref_build.py build(): a no-op where the reference tree is absent."""
    return ref_build.build()


def available() -> bool:
    return os.path.exists(LIB_PATH) or ref_build.have_reference()


def why_missing() -> str:
    return (f"{os.path.relpath(LIB_PATH, os.path.dirname(ref_build.HERE))} is not built and there is no reference "
            f"tree at {ref_build.reference_dir()} to build it from")


def lib():
    global _lib
    if _lib is None:
        if build() is None:
            raise RuntimeError(why_missing())
        L = C.CDLL(LIB_PATH)
        P = C.c_void_p
        f32, i32, u32, i64 = C.c_float, C.c_int32, C.c_uint32, C.c_int64
        L.ref_free.argtypes = [P]
        L.ref_read_ply.argtypes = [C.c_char_p, C.c_int, C.POINTER(P), C.POINTER(u32), C.POINTER(P)]
        L.ref_merge_sort.argtypes = [P, u32, C.c_int]
        L.ref_build_kd.argtypes = [P, u32, P, C.c_int]
        L.ref_camera_create.argtypes = [i32, i32, f32, f32, f32, P, P, P]
        L.ref_camera_create.restype = P
        L.ref_camera_destroy.argtypes = [P]
        L.ref_camera_basis.argtypes = [P, C.POINTER(OrcCamera)]
        L.ref_camera_rays.argtypes = [P, P]
        L.ref_host_vector_norm_n.argtypes = [P, i64, P]
        L.ref_device_inverse_sqrt_n.argtypes = [P, i64, P]
        L.ref_scene_create.argtypes = [i32, i32, f32, f32, f32, P, P, P, P, P, u32, P, P]
        L.ref_scene_create.restype = P
        L.ref_scene_destroy.argtypes = [P]
        L.ref_scene_set_xform.argtypes = [P, P]
        L.ref_scene_frame.argtypes = [P, C.c_int, P, P, P, P]
        L.ref_motion_tick.argtypes = [P, C.c_int]
        L.ref_motion_transform.argtypes = [P, P, C.c_int]
        L.ref_motion_state.argtypes = [P, P, P, P, P, P]
        for name in ("ref_free", "ref_merge_sort", "ref_camera_destroy", "ref_camera_basis", "ref_camera_rays",
                     "ref_host_vector_norm_n", "ref_device_inverse_sqrt_n", "ref_scene_destroy", "ref_scene_set_xform",
                     "ref_scene_frame", "ref_motion_tick", "ref_motion_transform", "ref_motion_state"):
            getattr(L, name).restype = None
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _f3(v):
    return np.ascontiguousarray(v, np.float32).reshape(3)


def _take(ptr, count, dtype):
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=dtype).copy()
    lib().ref_free(ptr)
    return arr


def read_ply(path: str, mode: int):
    """The reference's read_ply: -> (points9 [ntri, 9] f32, leafs LEAF_DTYPE;
    boxes and `tri` only, read_ply leaves the six sorted positions unset).
    It reads bodies after an `end_header` line and never ends on other files."""
    pts, lf, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
    lib().ref_read_ply(os.fsencode(path), mode, C.byref(pts), C.byref(n), C.byref(lf))
    leafs = _take(lf, n.value, LEAF_DTYPE)
    return _take(pts, 9 * n.value, np.float32).reshape(-1, 9), leafs


def merge_sort(leafs: np.ndarray, key: int) -> np.ndarray:
    a = np.ascontiguousarray(leafs, LEAF_DTYPE).copy()
    lib().ref_merge_sort(_ptr(a), len(a), key)
    return a


def build_kd(leafs: np.ndarray, fill: int = 0) -> np.ndarray:
    """Trixel(...), set_sorted_voxels, create_kd -> h_tree.h_nodes as NODE_DTYPE.
    The node array holds the byte `fill` before create_kd (the reference
    mallocs it): fields that differ between two fills were never written."""
    leafs = np.ascontiguousarray(leafs, LEAF_DTYPE)
    nodes = np.zeros(2 * len(leafs) - 1, NODE_DTYPE)
    lib().ref_build_kd(_ptr(leafs), len(leafs), _ptr(nodes), fill)
    return nodes


def _cam_args(w, h, f_w, f_h, focal, pos, look_at, up):
    from . import _oracle as O
    if f_w is None:
        f_w = O.film_w(w, h)
    return (w, h, np.float32(f_w), np.float32(f_h), np.float32(focal), _f3(pos), _f3(look_at), _f3(up))


def camera(w, h, f_w=None, f_h=0.024, focal=0.055, pos=(0.0, 0.1, -1.0), look_at=(0.0, 0.1, 0.0),
           up=(0.0, 1.0, 0.0)):
    """Camera(...) -> (its basis as an OrcCamera, the rmd plane [w * h, 3])."""
    a = _cam_args(w, h, f_w, f_h, focal, pos, look_at, up)
    c = lib().ref_camera_create(*a[:5], *[_ptr(v) for v in a[5:]])
    try:
        basis = OrcCamera()
        lib().ref_camera_basis(c, C.byref(basis))
        rays = np.zeros((w * h, 3), np.float32)
        lib().ref_camera_rays(c, _ptr(rays))
    finally:
        lib().ref_camera_destroy(c)
    return basis, rays


def host_vector_norm(s: np.ndarray) -> np.ndarray:
    s = np.ascontiguousarray(s, np.float32)
    out = np.zeros_like(s)
    lib().ref_host_vector_norm_n(_ptr(s), s.size, _ptr(out))
    return out


def device_inverse_sqrt(xyz: np.ndarray) -> np.ndarray:
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros(len(xyz), np.float32)
    lib().ref_device_inverse_sqrt_n(_ptr(xyz), len(xyz), _ptr(out))
    return out


class Scene:
    """A Camera, a Trixel and two Objects made in WinMain's order.  The tree is
    create_kd's over `leafs`, or `nodes` written in its place."""

    def __init__(self, w, h, points9, rad3, leafs=None, nodes=None, f_w=None, f_h=0.024, focal=0.055,
                 pos=(0.0, 0.1, -1.0), look_at=(0.0, 0.1, 0.0), up=(0.0, 1.0, 0.0)):
        assert (leafs is None) != (nodes is None)
        self.w, self.h, self.n = w, h, w * h
        self.points9 = np.ascontiguousarray(points9, np.float32).reshape(-1, 9)
        self.ntri = len(self.points9)
        self.rad3 = np.ascontiguousarray(rad3, np.float32).reshape(self.ntri, 3)
        self.leafs = None if leafs is None else np.ascontiguousarray(leafs, LEAF_DTYPE)
        self.nodes = None if nodes is None else np.ascontiguousarray(nodes, NODE_DTYPE)
        assert self.nodes is None or len(self.nodes) == 2 * self.ntri - 1
        self.cam_args = _cam_args(w, h, f_w, f_h, focal, pos, look_at, up)
        a = self.cam_args
        self._h = lib().ref_scene_create(*a[:5], *[_ptr(v) for v in a[5:]], _ptr(self.points9), _ptr(self.rad3),
                                         self.ntri, _ptr(self.leafs), _ptr(self.nodes))

    def set_xform(self, xform):
        x = np.ascontiguousarray(IDENT if xform is None else xform, np.float32).reshape(12)
        lib().ref_scene_set_xform(self._h, _ptr(x))

    def frame(self, mode=0):
        """One frame of the loop -> (hit [n] i64, aov [10, n] f32, shown [n] u32,
        clean [n] u32): the buffers after color_pixels(PHONG_COLOR_TAG), then
        h_color.c after color_pixels(SET_COLOR_TAG).  mode 1: the flat kernel."""
        assert mode == 1 or self.ntri > 1, "a one-triangle mesh has an index queue of length 0"
        hit = np.zeros(self.n, np.int64)
        aov = np.zeros((10, self.n), np.float32)
        shown = np.zeros(self.n, np.uint32)
        clean = np.zeros(self.n, np.uint32)
        lib().ref_scene_frame(self._h, mode, _ptr(hit), _ptr(aov), _ptr(shown), _ptr(clean))
        return hit, aov, shown, clean

    def tick(self, keys: int):
        lib().ref_motion_tick(self._h, keys)

    def transform(self, t_vec, select: int):
        t = np.ascontiguousarray(t_vec, np.float32).reshape(4)
        lib().ref_motion_transform(self._h, _ptr(t), select)

    def motion_state(self) -> dict:
        out = {k: np.zeros(n, np.float32) for k, n in (("rot_m", 12), ("d_rot_m", 12), ("quat", 4), ("init_face", 4),
                                                       ("cur_face", 4))}
        lib().ref_motion_state(self._h, *[_ptr(v) for v in out.values()])
        return out

    def close(self):
        if self._h:
            lib().ref_scene_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CASE_HEADER = "<2i3f3f3f3fI12f"   # oracle/ref_asan_main.cpp case_header


def write_case(path, w, h, points9, rad3, nodes, xform=None, f_w=None, f_h=0.024, focal=0.055,
               pos=(0.0, 0.1, -1.0), look_at=(0.0, 0.1, 0.0), up=(0.0, 1.0, 0.0)):
    """A render case for oracle/_ref/ref_asan (the host AddressSanitizer build)."""
    a = _cam_args(w, h, f_w, f_h, focal, pos, look_at, up)
    points9 = np.ascontiguousarray(points9, np.float32).reshape(-1, 9)
    n = len(points9)
    x = np.ascontiguousarray(IDENT if xform is None else xform, np.float32).reshape(12)
    with open(path, "wb") as fp:
        fp.write(struct.pack(CASE_HEADER, w, h, *[float(v) for v in a[2:5]], *a[5], *a[6], *a[7], n, *x))
        fp.write(points9.tobytes())
        fp.write(np.ascontiguousarray(rad3, np.float32).reshape(n, 3).tobytes())
        fp.write(np.ascontiguousarray(nodes, NODE_DTYPE).reshape(2 * n - 1).tobytes())
