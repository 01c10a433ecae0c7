"""Model-based random sequences of API operations on live cameras and scenes.

The kernels are stateless; the library around them (csrc/rt_api.cpp) is not:
cached launch geometry, gather rectangles, held fine regions, a ring of tile
orders, cost-order feedback, kept orders, shadow push-order tuning, per-stream
key buffers, camera records that follow a scene's tree, camera-owned planes.
The oracle has no state, so every render of any sequence of operations has a
known answer.  This module holds

  generate(seed)   a seeded list of operations (plain tuples, see OPERATIONS);
  Model            what each operation does to the state a render depends on,
                   which calls the ABI rejects, and which oracle frames a
                   render must equal (no GPU, no oracle call);
  Oracle           those frames, cached per (mesh, tree, camera, transform,
                   mode, shadow), and the ten hit planes from the hit index;
  Runner / replay  the operations on two cameras and seven scenes that stay
                   alive for the whole sequence, every render compared bit for
                   bit (needs a GPU; imported lazily).

tests/test_seq_cpu.py proves on the generator, the model and the oracle alone
that the sequences hold what they are there for; tests/test_gpu_sequences.py
runs them.

OPERATIONS (ci: camera index; every field an int or a string, so a list of
them is a Python literal and a JSON value):
  ("attach", ci, mesh)                 Camera.add_object of a new Object of that Trixel
  ("opt", ci, key, value)              Camera.set_option (valid, invalid and retired alike)
  ("sopt", mesh, key, value)           Trixel.set_option
  ("tree", mesh, name)                 Trixel.set_kd_nodes: a tree of TREES[mesh] or one of BAD_TREES
  ("build", mesh)                      Trixel.create_kd(on_device=True)
  ("xf", ci, name)                     the object's transform, one of XF_NAMES
  ("tick", ci, keys)                   Object.key_tick
  ("sync", s)                          stream s synchronised, -1: the device
  ("render", ci, mode, flags, target)  target: ("own",) | ("into", s) | ("ranks", nranks, s)
                                       | ("over", mesh2, s) | ("display", s)
                                       | ("xshadow", mesh2, s, skip_own, first)
                                       (s: one of NSTREAMS torch streams; "own": Object.render into the
                                       camera's buffers; "ranks": every rank's band tile, then unpack_bands;
                                       "over": clear_layers, render_over, add_object(mesh2), render_over;
                                       "display": render_display against oracle.Window;
                                       "xshadow": the "over" target, then the two objects' deferred shadow
                                       passes (Camera.shadow_over) over the same targets on stream s, each
                                       object attached again for its pass with the transform it was rendered
                                       with and its hit base, object `first` (0: the base, 1: mesh2) first;
                                       with skip_own the two renders carry SHADOW; flags: COUNT or none; the
                                       camera then shows mesh2 at the identity, as "over" leaves it.  KD only:
                                       the generator emits a flat one only with skip_own, whose flat SHADOW
                                       render is the rejection "xshadow_flat")
  ("shadow", ci, s)                    Camera.shadow_over with no targets: the pass over the camera's own
                                       frame, hit index and planes (rejected until a render filled the planes)
  ("loop", ci, mode, flags, nframes, inflight, nbuf, s)   FrameLoop.run
"""
import numpy as np

from oracle import _oracle as O, motion as M, np_oracle as N
from tests import helpers as H, synth as S
from tests.synth import SPLIT_FIELD_VARIANTS

F = np.float32
D = np.float64

CAMS = ((96, 54), (33, 19))        # 6 x 7 KD tiles of 16 x 8, 3 x 7 flat tiles of 32 x 8, 7 bands | one odd small frame
MESHES = ("s257", "s33", "s9", "s1", "copies", "grid", "mat")
NTRI = {"s257": 257, "s33": 33, "s9": 9, "s1": 1, "copies": S.COPIES[0] * S.COPIES[1], "grid": 28, "mat": S.LIGHT_N}
TREES = {m: ("built",) for m in MESHES} | {
    "s33": ("built", "swapped", "inflated", "shrunk") + S.SPLIT_FIELD_VARIANTS}
BAD_TREES = ("bad_dup", "bad_bfs", "bad_count")
NSTREAMS = 10
MULTIFRAME = -1                    # RT_LOOP_MULTIFRAME

HIT, COUNT, SHADOW, AOV = 1, 2, 4, 16
KD, FLAT = 0, 1

# camera option keys (include/rt_mi355x.h) and the values the sequences set
K_KERNEL, K_ORDER, K_RAYS, K_ITEMS, K_COARSE, K_SHADOW_ORDER, K_FLAT, K_DEBUG, K_POOL = 1, 2, 3, 4, 5, 6, 7, 100, 101
DEBUG_BITS = (4, 8, 64, 256, 1024, 2048)   # the frame-preserving bits the other suites use
OPT_VALUES = {K_KERNEL: (2, 3), K_ORDER: (0, 1, 2, 3, 4, 5), K_RAYS: (0, 8, 16, 32), K_ITEMS: (1, 2, 96),
              K_COARSE: (0, 1, 8, 32), K_FLAT: (9, 12), K_POOL: (89, 96, 640), K_SHADOW_ORDER: (-1, 0, 1, 2, 3)}
OPT_BAD = {K_KERNEL: (1, 4), K_ORDER: (-1, 6), K_RAYS: (4, 64), K_ITEMS: (0, 3, 64), K_COARSE: (-1, 33),
           K_FLAT: (0, 10, 13), K_POOL: (88, 641), K_SHADOW_ORDER: (-2, 4)}
OPT_RETIRED = (10, 11)
OPT_DEFAULTS = {K_KERNEL: 3, K_ORDER: 3, K_RAYS: 0, K_ITEMS: 2, K_COARSE: 8, K_FLAT: 12, K_POOL: 640,
                K_SHADOW_ORDER: -1, K_DEBUG: 0}
OPT_READABLE = (K_KERNEL, K_ORDER, K_RAYS, K_ITEMS, K_COARSE, K_FLAT, K_DEBUG)   # rt_camera_get_option returns the set value
S_ORDER, S_HEIGHT = 1, 2           # RT_SCENE_ORDER, RT_SCENE_TREELET_HEIGHT
SOPT_VALUES = {S_ORDER: (0, 1, 2), S_HEIGHT: (1, 2, 3, 4, 5)}
SOPT_DEFAULTS = {S_ORDER: 0, S_HEIGHT: 3}
TICKS = (M.KEY_W, M.KEY_R, M.KEY_W | M.KEY_Q, M.KEY_T | M.KEY_S, M.KEY_E, M.KEY_R | M.KEY_W, M.KEY_Q, M.KEY_T)

IDENT = tuple(float(x) for x in N.IDENT)

REJECTIONS = ("opt_value", "opt_retired", "tree_dup", "tree_bfs", "tree_count", "shadow_flat", "shadow_k2", "flags_high",
              "loop_aov", "xshadow_flat", "xshadow_k2", "xshadow_flags", "shadow_unfilled")
#: the RtError code include/rt_mi355x.h documents for the deferred pass's rejections (RT_ERR_INVALID -1, RT_ERR_STATE -5)
REJECT_CODES = {"xshadow_flat": -1, "xshadow_k2": -1, "xshadow_flags": -1, "shadow_unfilled": -5}
STATE_KINDS = ("opt", "opt_bad", "sopt", "tree", "tree_bad", "build", "attach", "xf", "tick", "sync", "loop")
TARGETS = ("own", "into", "ranks", "over", "display", "xshadow")
RENDER_KINDS = tuple(f"{t}/{m}" for t in TARGETS + ("loop",) for m in ("kd", "flat") if (t, m) != ("xshadow", "flat"))
XSHADOW_CAM0_CAP = 2               # "xshadow" renders per sequence on the 96x54 camera (the numpy reference's cost)
SEEDS = (101, 102, 103, 104, 105, 106, 107, 108)


def xforms():
    """name -> transform (12 floats): the identity, rot_y(17), the small
    translation, test_gpu_parity's general rotations and the signed permutation."""
    from tests.test_gpu_parity import _GENERAL_XFS
    out = {"id": N.IDENT, "rot": S.rot_y(17.0), "xlate": S.rot_y(0.0, (0.01, -0.005, 0.02)), "perm": S.SIGNED_PERM}
    out |= {f"gen{k}": _GENERAL_XFS[k] for k in range(5)}
    return {k: tuple(float(x) for x in np.asarray(v, F).reshape(12)) for k, v in out.items()}


XF_NAMES = ("id", "rot", "xlate", "perm", "gen0", "gen1", "gen2", "gen3", "gen4")
_xfs = None


def xform_of(name):
    global _xfs
    if _xfs is None:
        _xfs = xforms()
        assert tuple(_xfs) == XF_NAMES
    return _xfs[name]


def _norm(op):
    """An operation as nested tuples (JSON gives lists)."""
    return tuple(_norm(x) if isinstance(x, (list, tuple)) else x for x in op)


# ----------------------------------------------------------------------- model

def opt_valid(key, value):
    """Whether rt_camera_set_option documents (key, value) as accepted."""
    if key == K_DEBUG:
        return True
    if key == K_ITEMS:
        return value in (1, 2) or 65 <= value <= 128
    if key == K_COARSE:
        return 0 <= value <= 32
    if key == K_POOL:
        return 89 <= value <= 640
    if key == K_SHADOW_ORDER:
        return -1 <= value <= 3
    if key == K_ORDER:
        return 0 <= value <= 5
    return key in OPT_VALUES and value in OPT_VALUES[key]


class Exp:
    """What the model expects of one operation.
      kind     the operation's kind: a STATE_KINDS entry, or "render"
      reject   None, or the REJECTIONS entry the call must fail with (RtError)
      cams     the cameras whose next render the operation bears on
      rkind    a render's / loop's RENDER_KINDS entry
      layers   a valid render's frames: [(spec, hit_base)], spec = (mesh, tree,
               ci, transform, mode, shadow) (Oracle.frame / Oracle.planes)
      snap     the camera state a render ran in (conditions of test_seq_cpu.py)
      xshadow  None, or (skip_own, first) of a composite whose deferred shadow
               passes ran (the frame is then Oracle.cross's)"""

    def __init__(self, op, kind, reject=None, cams=(), rkind=None, layers=(), snap=None, xshadow=None):
        self.op, self.kind, self.reject, self.cams, self.rkind = op, kind, reject, tuple(cams), rkind
        self.layers, self.snap, self.xshadow = list(layers), snap, xshadow


class _Cam:
    def __init__(self, w, h):
        self.w, self.h = w, h
        self.opts = dict(OPT_DEFAULTS)
        self.mesh = None
        self.xf = IDENT
        self.motion = None
        self.gen = 0           # bumps whenever anything a render of this camera depends on changes
        self.aov_filled = False   # a render wrote the camera's own planes (never cleared)
        self.own = dict(argb=None, hit=None, aov=None)   # the specs the camera's own buffers hold


class Model:
    def __init__(self):
        self.cams = [_Cam(w, h) for w, h in CAMS]
        self.tree = {m: "built" for m in MESHES}
        self.sopts = {m: dict(SOPT_DEFAULTS) for m in MESHES}
        self._ncam = None

    def _np_cam(self, ci):
        if self._ncam is None:
            self._ncam = [N.camera(w, h) for w, h in CAMS]
        return self._ncam[ci]

    def on(self, mesh):
        """The cameras that show `mesh`."""
        return [ci for ci, c in enumerate(self.cams) if c.mesh == mesh]

    def _attach(self, ci, mesh):
        c = self.cams[ci]
        nc = self._np_cam(ci)
        c.mesh, c.xf = mesh, IDENT            # Camera.add_object: a new Quaternion and motion state
        c.motion = M.Motion(nc["pos"], nc["n"], nc["u"])
        c.gen += 1

    def render_reject(self, ci, mode, flags, loop=False):
        c = self.cams[ci]
        if flags & ~31:
            return "flags_high"
        if loop and flags & AOV:
            return "loop_aov"
        if flags & SHADOW and mode != KD:
            return "shadow_flat"
        if flags & SHADOW and c.opts[K_KERNEL] != 3:
            return "shadow_k2"
        return None

    def xshadow_reject(self, ci, mode, flags, skip_own):
        """An "xshadow" render's rejection, by the first call that fails: the
        render (flags_high; xshadow_flat: SHADOW in flat mode) or the pass
        (xshadow_k2: kernel 2; xshadow_flags: any flag but COUNT / FRAME_OUT)."""
        if flags & ~31:
            return "flags_high"
        if mode != KD:
            assert skip_own, "a flat xshadow without skip_own is not an operation"
            return "xshadow_flat"
        if self.cams[ci].opts[K_KERNEL] != 3:
            return "xshadow_k2"
        if flags & ~(COUNT | 8):
            return "xshadow_flags"
        assert not flags & 8, "RT_FLAG_FRAME_OUT is not generated"
        return None

    def _snap(self, ci, mode, flags, nranks=1, stream=None):
        c = self.cams[ci]
        o = c.opts
        return dict(ci=ci, mesh=c.mesh, tree=self.tree[c.mesh], kernel=o[K_KERNEL], order=o[K_ORDER], flat=o[K_FLAT],
                    mode=mode, flags=flags, stream=stream, gen=c.gen, xf=c.xf, shadow_order=o[K_SHADOW_ORDER],
                    items=o[K_ITEMS], pool=o[K_POOL], debug=o[K_DEBUG],
                    grid=(c.mesh, c.xf, o[K_KERNEL], o[K_RAYS], o[K_COARSE], o[K_DEBUG], mode, nranks))

    def _spec(self, ci, mode, flags):
        c = self.cams[ci]
        # (the flat list takes neither the tree nor the transform)
        return (c.mesh, self.tree[c.mesh] if mode == KD else "-", ci, c.xf if mode == KD else IDENT, mode,
                bool(flags & SHADOW))

    def step(self, op):
        op = _norm(op)
        k = op[0]
        if k == "attach":
            _, ci, mesh = op
            self._attach(ci, mesh)
            return Exp(op, "attach", cams=[ci])
        if k == "opt":
            _, ci, key, value = op
            if key in OPT_RETIRED:
                return Exp(op, "opt_bad", "opt_retired", cams=[ci])
            if not opt_valid(key, value):
                return Exp(op, "opt_bad", "opt_value", cams=[ci])
            self.cams[ci].opts[key] = value
            self.cams[ci].gen += 1
            return Exp(op, "opt", cams=[ci])
        if k == "sopt":
            _, mesh, key, value = op
            assert value in SOPT_VALUES[key]
            self.sopts[mesh][key] = value
            for ci in self.on(mesh):
                self.cams[ci].gen += 1
            return Exp(op, "sopt", cams=self.on(mesh))
        if k == "tree":
            _, mesh, name = op
            if name in BAD_TREES:
                return Exp(op, "tree_bad", "tree_" + name[4:], cams=self.on(mesh))
            assert name in TREES[mesh]
            self.tree[mesh] = name
            for ci in self.on(mesh):
                self.cams[ci].gen += 1
            return Exp(op, "tree", cams=self.on(mesh))
        if k == "build":
            _, mesh = op
            self.tree[mesh] = "built"
            for ci in self.on(mesh):
                self.cams[ci].gen += 1
            return Exp(op, "build", cams=self.on(mesh))
        if k == "xf":
            _, ci, name = op
            self.cams[ci].xf = xform_of(name)
            self.cams[ci].gen += 1
            return Exp(op, "xf", cams=[ci])
        if k == "tick":
            _, ci, keys = op
            c = self.cams[ci]
            c.motion.tick(keys)
            c.xf = tuple(float(x) for x in c.motion.xform())
            c.gen += 1
            return Exp(op, "tick", cams=[ci])
        if k == "sync":
            return Exp(op, "sync", cams=range(len(self.cams)))
        if k == "render":
            _, ci, mode, flags, target = op
            c = self.cams[ci]
            assert c.mesh is not None and mode in (KD, FLAT) and target[0] in TARGETS
            rkind = f"{target[0]}/{'flat' if mode else 'kd'}"
            nranks = target[1] if target[0] == "ranks" else 1
            snap = self._snap(ci, mode, flags, nranks, target[2] if target[0] == "xshadow" else
                              target[-1] if target[0] != "own" else None)
            if target[0] == "xshadow":
                _, mesh2, _, skip_own, first = target
                rej = self.xshadow_reject(ci, mode, flags, skip_own)
                if rej:
                    return Exp(op, "render", rej, cams=[ci], rkind=rkind, snap=snap)
                rflags = flags | (SHADOW if skip_own else 0)
                layers = [(self._spec(ci, mode, rflags), 0)]
                self._attach(ci, mesh2)           # the second layer's object, at the identity
                layers.append((self._spec(ci, mode, rflags), NTRI[layers[0][0][0]]))
                return Exp(op, "render", cams=[ci], rkind=rkind, layers=layers, snap=snap, xshadow=(skip_own, first))
            rej = self.render_reject(ci, mode, flags)
            if rej:
                return Exp(op, "render", rej, cams=[ci], rkind=rkind, snap=snap)
            layers = [(self._spec(ci, mode, flags), 0)]
            if target[0] == "own":
                c.own["argb"] = layers[0][0]
                if flags & (HIT | AOV):           # (the planes ride on the write-hit instances)
                    c.own["hit"] = layers[0][0][:5]
                if flags & AOV:
                    c.own["aov"], c.aov_filled = layers[0][0][:5], True
            if target[0] == "over":
                base = NTRI[c.mesh]
                self._attach(ci, target[1])       # the second layer's object, at the identity
                layers.append((self._spec(ci, mode, flags), base))
            return Exp(op, "render", cams=[ci], rkind=rkind, layers=layers, snap=snap)
        if k == "loop":
            _, ci, mode, flags, nframes, inflight, nbuf, s = op
            assert self.cams[ci].mesh is not None and 1 <= nbuf <= nframes and inflight in (1, 2, MULTIFRAME)
            assert inflight != 2 or nbuf % 2 == 0
            rkind = f"loop/{'flat' if mode else 'kd'}"
            snap = self._snap(ci, mode, flags, 1, s) | dict(nframes=nframes, inflight=inflight)
            rej = self.render_reject(ci, mode, flags, loop=True)
            if rej:
                return Exp(op, "loop", rej, cams=[ci], rkind=rkind, snap=snap)
            return Exp(op, "loop", cams=[ci], rkind=rkind, layers=[(self._spec(ci, mode, flags), 0)], snap=snap)
        if k == "shadow":
            _, ci, s = op
            c = self.cams[ci]
            if c.opts[K_KERNEL] != 3:
                return Exp(op, "shadow", "xshadow_k2", cams=[ci])
            if not c.aov_filled:
                return Exp(op, "shadow", "shadow_unfilled", cams=[ci])
            spec = c.own["argb"]
            # the camera's own frame, hit index and planes are one KD render's, of the object it shows now
            assert spec is not None and c.own["hit"] == c.own["aov"] == spec[:5] and spec[4] == KD, (op, c.own)
            assert spec[:4] == (c.mesh, self.tree[c.mesh], ci, c.xf), (op, spec)
            c.own["argb"] = spec[:5] + (True,)
            return Exp(op, "shadow", cams=[ci], layers=[(c.own["argb"], 0)])
        raise ValueError(f"unknown operation {op!r}")


def trace(ops):
    """The model's expectation of every operation of a sequence."""
    m = Model()
    return [m.step(op) for op in ops]


# ------------------------------------------------------------------ generator

class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng([seed, 0x5E9])
        self.seed = seed
        self.m = Model()
        self.ops = []
        self.x0 = 0            # "xshadow" renders on camera 0 so far (XSHADOW_CAM0_CAP)

    # -- helpers
    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def emit(self, *op):
        e = self.m.step(op)
        self.ops.append(e.op)
        if e.xshadow and e.op[1] == 0:
            self.x0 += 1
        return e

    def cam(self):
        return int(self.rng.integers(len(CAMS)))

    def xcam(self, need=1):
        """A camera for `need` "xshadow" renders: the large one while its budget lasts."""
        return self.cam() if self.x0 + need <= XSHADOW_CAM0_CAP else 1

    def flags(self, ci, mode, allow=(HIT, COUNT, SHADOW, AOV)):
        f = 0
        for bit in allow:
            if self.rng.random() < 0.5:
                f |= bit
        if self.m.render_reject(ci, mode, f):
            f &= ~SHADOW
        return f

    def target(self, kind=None, ci=1):
        if kind is None:
            kind = self.pick(TARGETS)
            if kind == "xshadow" and ci == 0 and self.x0 >= XSHADOW_CAM0_CAP:
                kind = "over"
        s = int(self.rng.integers(NSTREAMS))
        if kind == "xshadow":     # (257 triangles as the second layer of the large camera: the reference's slowest pair)
            return ("xshadow", self.pick(MESHES[1:] if ci == 0 else MESHES), s, int(self.rng.integers(2)),
                    int(self.rng.integers(2)))
        if kind == "own":
            return ("own",)
        if kind == "ranks":
            return ("ranks", self.pick((2, 3, 8)), s)
        if kind == "over":
            return ("over", self.pick(MESHES), s)
        return (kind, s)

    def render(self, ci, kind=None, mode=None, flags=None, target=None):
        mode = self.pick((KD, KD, FLAT)) if mode is None else mode
        target = target or self.target(kind, ci)
        if target[0] == "xshadow":           # a valid one: KD, kernel 3, COUNT or no flag
            assert ci == 1 or self.x0 < XSHADOW_CAM0_CAP
            self.ensure(ci, K_KERNEL, (3,))
            mode, flags = KD, self.pick((0, COUNT)) if flags is None else flags
        self.emit("render", ci, mode, self.flags(ci, mode) if flags is None else flags, target)

    def loop(self, ci, mode=None, inflight=None, flags=None, nframes=None):
        mode = self.pick((KD, KD, FLAT)) if mode is None else mode
        inflight = self.pick((1, 2, MULTIFRAME)) if inflight is None else inflight
        nbuf = 2 if inflight != 1 else self.pick((1, 2))
        nframes = int(self.rng.integers(3, 41)) if nframes is None else nframes
        flags = self.flags(ci, mode, allow=(COUNT, SHADOW)) if flags is None else flags
        self.emit("loop", ci, mode, flags, nframes, inflight, nbuf, int(self.rng.integers(NSTREAMS)))

    def any_render(self, ci, rkind):
        t, m = rkind.split("/")
        mode = FLAT if m == "flat" else KD
        if t == "loop":
            self.loop(ci, mode=mode)
        else:
            self.render(ci, kind=t, mode=mode)

    def other_tree(self, mesh):
        names = [n for n in TREES[mesh] if n != self.m.tree[mesh]] or ["built"]
        return self.pick(names)

    def other_mesh(self, ci, differ=True):
        cur = self.m.cams[ci].mesh
        return self.pick([m for m in MESHES if not differ or cur is None or NTRI[m] != NTRI[cur]])

    def debug_value(self):
        return int(sum(b for b in DEBUG_BITS if self.rng.random() < 0.3))

    def state_op(self, kind, ci, keep_kernel=False):
        """One state-changing operation of `kind` that bears on camera ci."""
        mesh = self.m.cams[ci].mesh
        if kind == "opt":
            key = self.pick(tuple(OPT_VALUES) + (K_DEBUG, K_ORDER, K_KERNEL))
            while keep_kernel and key == K_KERNEL:
                key = self.pick(tuple(OPT_VALUES))
            self.emit("opt", ci, key, self.debug_value() if key == K_DEBUG else self.pick(OPT_VALUES[key]))
        elif kind == "opt_bad":
            if self.rng.random() < 0.3:
                self.emit("opt", ci, self.pick(OPT_RETIRED), int(self.rng.integers(0, 4)))
            else:
                key = self.pick(tuple(OPT_BAD))
                self.emit("opt", ci, key, self.pick(OPT_BAD[key]))
        elif kind == "sopt":
            key = self.pick((S_ORDER, S_ORDER, S_HEIGHT))
            self.emit("sopt", mesh, key, self.pick([v for v in SOPT_VALUES[key] if v != self.m.sopts[mesh][key]]))
        elif kind == "tree":
            self.emit("tree", mesh, self.other_tree(mesh))
        elif kind == "tree_bad":
            self.emit("tree", mesh, self.pick(BAD_TREES))
        elif kind == "build":
            self.emit("build", mesh)
        elif kind == "attach":
            self.emit("attach", ci, self.other_mesh(ci))
        elif kind == "xf":
            # (the far rotations and the permutation leave few or no hit pixels: the near ones twice as often)
            self.emit("xf", ci, self.pick(XF_NAMES + ("id", "rot", "xlate", "gen0", "gen3", "rot", "xlate")))
        elif kind == "tick":
            self.emit("tick", ci, self.pick(TICKS))
        elif kind == "sync":
            self.emit("sync", int(self.rng.integers(-1, NSTREAMS)))
        elif kind == "loop":
            self.loop(ci)
        else:
            raise ValueError(kind)

    def ensure(self, ci, key, values):
        if self.m.cams[ci].opts[key] not in values:
            self.emit("opt", ci, key, self.pick(values))

    # -- episodes: the transitions test_seq_cpu.py's conditions name
    def ep_a(self):
        """A cost order measured over frames with a sync among them, a new tree, the same grid again."""
        ci = self.cam()
        if self.rng.random() < 0.6 and self.m.cams[ci].mesh != "s33":
            self.emit("attach", ci, "s33")      # the mesh with hand-made trees
        self.ensure(ci, K_KERNEL, (3,))
        self.emit("opt", ci, K_ORDER, self.pick((3, 4)))
        s = int(self.rng.integers(NSTREAMS))
        t = ("into", s)
        for _ in range(2):
            self.render(ci, mode=KD, flags=self.pick((0, HIT)), target=t)
        self.emit("sync", self.pick((-1, s)))
        if self.rng.random() < 0.5:
            self.emit("loop", ci, KD, 0, int(self.rng.integers(17, 41)), 1, 1, s)
            self.emit("sync", -1)
        self.render(ci, mode=KD, flags=self.pick((0, HIT)), target=t)
        mesh = self.m.cams[ci].mesh
        if self.rng.random() < 0.3:
            self.emit("build", mesh)
        else:
            self.emit("tree", mesh, self.other_tree(mesh))
        self.render(ci, mode=KD, flags=self.pick((0, HIT, HIT | COUNT)), target=t)

    def ep_b(self):
        ci = self.cam()
        self.render(ci, mode=FLAT)
        self.emit("attach", ci, self.other_mesh(ci))
        self.render(ci, mode=FLAT)

    def ep_c(self):
        ci = self.cam()
        for mesh in ("s257", "s1", "s257"):
            if self.m.cams[ci].mesh != mesh:
                self.emit("attach", ci, mesh)
            self.render(ci, mode=KD)
            if mesh == "s1":
                self.render(ci, kind=self.pick(("own", "into")), mode=KD, flags=self.pick((HIT, HIT | COUNT)))
                self.render(ci, mode=FLAT)

    def ep_d(self):
        mesh = self.pick(("s257", "s33", "copies", "grid", "mat", "s9"))
        for ci in range(len(CAMS)):
            if self.m.cams[ci].mesh != mesh:
                self.emit("attach", ci, mesh)
        single = ("own", "into", "ranks", "display")     # (a composite ends on another object)
        for ci in range(len(CAMS)):
            self.render(ci, kind=self.pick(single), mode=KD)
        self.emit("sopt", mesh, S_ORDER, self.pick([v for v in (0, 1, 2) if v != self.m.sopts[mesh][S_ORDER]]))
        for ci in range(len(CAMS)):
            self.render(ci, kind=self.pick(single), mode=KD)

    def ep_e(self):
        ci = self.cam()
        self.ensure(ci, K_KERNEL, (3,))
        self.ensure(ci, K_ORDER, (2, 3, 4, 5))
        for s in self.rng.permutation(NSTREAMS):
            self.render(ci, mode=KD, flags=self.pick((0, HIT)), target=("into", int(s)))
        self.ensure(ci, K_FLAT, (12,))
        for s in self.rng.permutation(NSTREAMS):
            self.render(ci, mode=FLAT, flags=self.pick((0, HIT)), target=("into", int(s)))

    def ep_f(self):
        ci = 1
        self.ensure(ci, K_KERNEL, (3,))
        self.loop(ci, mode=KD, inflight=MULTIFRAME, flags=0)
        self.render(ci, mode=KD)
        self.loop(ci, mode=KD, inflight=MULTIFRAME, flags=0)

    def ep_h(self):
        """Two tilings of the small camera with a cost order each (the
        multi-frame rule's rays per wave and the per-frame one's), a new tree,
        the first tiling again: no kept order may come back."""
        ci = 1
        self.ensure(ci, K_KERNEL, (3,))
        self.emit("opt", ci, K_ORDER, 3)
        self.ensure(ci, K_RAYS, (0,))
        s = int(self.rng.integers(NSTREAMS))
        self.emit("loop", ci, KD, 0, 40, MULTIFRAME, 2, s)
        self.emit("sync", -1)
        self.emit("loop", ci, KD, 0, 8, MULTIFRAME, 2, s)
        for _ in range(3):
            self.render(ci, mode=KD, flags=self.pick((0, HIT)), target=("into", s))
            self.emit("sync", s)
        mesh = self.m.cams[ci].mesh
        if self.rng.random() < 0.3:
            self.emit("build", mesh)
        else:
            self.emit("tree", mesh, self.other_tree(mesh))
        self.emit("loop", ci, KD, 0, 8, MULTIFRAME, 2, s)

    def ep_reject(self, kind):
        """A rejected call, then a valid one with the same targets."""
        ci = self.cam()
        mesh = self.m.cams[ci].mesh
        if kind in ("opt_value", "opt_retired"):
            if kind == "opt_retired":
                self.emit("opt", ci, self.pick(OPT_RETIRED), int(self.rng.integers(0, 4)))
            else:
                key = self.pick(tuple(OPT_BAD))
                self.emit("opt", ci, key, self.pick(OPT_BAD[key]))
            self.render(ci)
        elif kind.startswith("tree_"):
            self.emit("tree", mesh, "bad_" + kind[5:])
            self.render(ci, mode=KD)                 # the previous tree keeps rendering
        elif kind == "loop_aov":
            s = int(self.rng.integers(NSTREAMS))
            inflight = self.pick((1, 2, MULTIFRAME))
            self.emit("loop", ci, KD, AOV | self.pick((0, COUNT)), 5, inflight, 2, s)
            self.emit("loop", ci, KD, 0, 5, inflight, 2, s)
        else:
            target = self.target()
            if kind == "shadow_k2":
                self.ensure(ci, K_KERNEL, (2,))
                mode, flags = KD, SHADOW | self.flags(ci, KD, allow=(HIT, COUNT, AOV))
            elif kind == "shadow_flat":
                mode, flags = FLAT, SHADOW | self.flags(ci, FLAT, allow=(HIT, COUNT, AOV))
            else:
                mode = self.pick((KD, FLAT))
                flags = self.pick((32, 64, 128, 1 << 30)) | self.flags(ci, mode)
            if target[0] == "xshadow":       # (the pass's own rejections are ep_reject_x's)
                target = ("over",) + target[1:3]
            self.emit("render", ci, mode, flags, target)
            self.emit("render", ci, mode, self.flags(ci, mode) & ~SHADOW, target)

    def ep_reject_x(self, kind):
        """A rejected deferred pass, then a valid "xshadow" with the same targets."""
        ci = self.xcam()
        t = self.target("xshadow", ci)
        if kind == "xshadow_flat":
            self.emit("render", ci, FLAT, self.pick((0, COUNT)), t[:3] + (1, t[4]))
        elif kind == "xshadow_k2":
            self.ensure(ci, K_KERNEL, (2,))
            self.emit("render", ci, KD, self.pick((0, COUNT)), t)
        else:
            self.ensure(ci, K_KERNEL, (3,))
            self.emit("render", ci, KD, self.pick((HIT, SHADOW, AOV, HIT | COUNT, AOV | HIT | SHADOW)), t)
        self.render(ci, target=t)

    # -- episodes of the deferred shadow pass (test_seq_cpu.py's x_* conditions)
    def xshadow(self, ci, mesh2=None, flags=None, skip_own=None, first=None, s=None):
        t = self.target("xshadow", ci)
        t = ("xshadow", t[1] if mesh2 is None else mesh2, t[2] if s is None else s, t[3] if skip_own is None else skip_own,
             t[4] if first is None else first)
        self.render(ci, mode=KD, flags=flags, target=t)

    def ep_x_own(self):
        """The pass over the camera's own buffers, right after the render that filled them."""
        ci = self.cam()
        self.ensure(ci, K_KERNEL, (3,))
        self.emit("render", ci, KD, HIT | AOV | self.pick((0, COUNT, SHADOW)), ("own",))
        self.emit("shadow", ci, int(self.rng.integers(NSTREAMS)))

    def ep_x_timed(self):
        """A timed round of the shadow push order (12 trial frames and the one
        that reads them), then the passes under the order it chose."""
        ci = self.xcam()
        self.ensure(ci, K_KERNEL, (3,))
        self.emit("opt", ci, K_SHADOW_ORDER, -1)
        s = int(self.rng.integers(NSTREAMS))
        self.emit("loop", ci, KD, SHADOW, int(self.rng.integers(13, 20)), 1, 1, s)
        self.emit("sync", -1)
        self.render(ci, mode=KD, flags=SHADOW | self.pick((0, HIT)), target=("into", s))
        self.xshadow(ci, s=s)

    def ep_x_cost(self):
        """The passes between two cost-order renders of one grid."""
        ci = self.xcam()
        self.ensure(ci, K_KERNEL, (3,))
        self.emit("opt", ci, K_ORDER, self.pick((3, 4)))
        if self.m.cams[ci].xf != IDENT:
            self.emit("xf", ci, "id")
        t = ("into", int(self.rng.integers(NSTREAMS)))
        self.render(ci, mode=KD, flags=self.pick((0, HIT, HIT | COUNT)), target=t)
        self.xshadow(ci, mesh2=self.m.cams[ci].mesh)
        self.render(ci, mode=KD, flags=self.pick((HIT, HIT | COUNT)), target=t)

    def ep_x_after(self, kind):
        """The passes right after a tree replacement (a split-field variant), a device build or a scene option."""
        ci = self.xcam()
        self.ensure(ci, K_KERNEL, (3,))
        if kind == "tree":
            if self.m.cams[ci].mesh != "s33":
                self.emit("attach", ci, "s33")
            self.emit("tree", "s33", self.pick([n for n in SPLIT_FIELD_VARIANTS if n != self.m.tree["s33"]]))
        elif kind == "build":
            self.emit("build", self.m.cams[ci].mesh)
        else:
            self.state_op("sopt", ci)
        self.xshadow(ci)

    def ep_x_opts(self):
        """The passes under the smallest pool, one item per lane and debug bit 16."""
        ci = self.xcam(3)
        self.ensure(ci, K_KERNEL, (3,))
        self.emit("opt", ci, K_POOL, 89)
        self.xshadow(ci)
        self.emit("opt", ci, K_ITEMS, 1)
        self.xshadow(ci)
        debug = self.m.cams[ci].opts[K_DEBUG]
        self.emit("opt", ci, K_DEBUG, debug | 16)
        self.xshadow(ci, flags=0)            # (a counted walk under bit 16 stops at occluders: no counters to compare)
        self.emit("opt", ci, K_DEBUG, debug)

    def ep_ticks(self):
        """A moving object: a run of key ticks, a render after each."""
        ci = self.cam()
        kind = self.pick(("own", "into"))
        for _ in range(int(self.rng.integers(3, 7))):
            self.emit("tick", ci, self.pick(TICKS))
            self.render(ci, kind=kind, mode=KD)

    def ep_opts(self, settings):
        """Option values (every settable one once over eight consecutive seeds), a render after each."""
        ci = self.cam()
        for key, value in settings:
            self.emit("opt", ci, key, value)
            if key == K_FLAT:
                self.render(ci, mode=FLAT)
            elif key == K_SHADOW_ORDER:
                self.ensure(ci, K_KERNEL, (3,))
                self.render(ci, mode=KD, flags=SHADOW | self.flags(ci, KD, allow=(HIT, COUNT)))
            else:
                if key != K_KERNEL:
                    self.ensure(ci, K_KERNEL, (3, 3, 2) if key in (K_ORDER, K_DEBUG) else (3,))
                self.render(ci, mode=KD)

    def ep_sopt(self, key, value):
        ci = self.cam()
        mesh = self.m.cams[ci].mesh
        if key == S_HEIGHT and self.m.sopts[mesh][S_ORDER] != 2:
            self.emit("sopt", mesh, S_ORDER, 2)       # the treelet order is the one that reads the height
        self.emit("sopt", mesh, key, value)
        self.render(ci, mode=KD)

    def ep_xf(self, name):
        ci = self.cam()
        self.emit("xf", ci, name)
        self.render(ci, mode=KD)
        self.render(ci, kind=self.pick(("own", "into", "ranks")), mode=KD, flags=self.flags(ci, KD) | HIT)

    def ep_tree(self, name):
        """A hand-made tree under a camera that has rendered the scene."""
        ci = self.cam()
        if self.m.cams[ci].mesh != "s33":
            self.emit("attach", ci, "s33")
        self.render(ci, mode=KD)
        if self.m.tree["s33"] == name:
            self.emit("tree", "s33", self.other_tree("s33"))
        self.emit("tree", "s33", name)
        self.render(ci, mode=KD, flags=HIT | COUNT | self.flags(ci, KD, allow=(SHADOW, AOV)))
        self.render(ci, mode=KD)

    def filler(self):
        ci = self.cam()
        self.state_op(self.pick(STATE_KINDS), ci)
        if self.rng.random() < 0.8:
            self.render(ci)

    def pair(self, skind, rkind):
        if rkind.startswith("xshadow"):      # kernel 3 first: the state change is then the last thing before the passes
            ci = self.xcam()
            self.ensure(ci, K_KERNEL, (3,))
            self.state_op(skind, ci, keep_kernel=True)
        else:
            ci = self.cam()
            self.state_op(skind, ci)
        self.any_render(ci, rkind)

    def run(self):
        self.emit("attach", 0, "s257")
        self.emit("attach", 1, self.pick(("s33", "copies", "mat")))
        self.emit("shadow", self.cam(), int(self.rng.integers(NSTREAMS)))   # nothing has filled the camera's own planes
        # every (state kind, render kind) pair once over eight consecutive seeds
        deck = [(s, r) for s in STATE_KINDS for r in RENDER_KINDS]
        np.random.default_rng(0x5E9).shuffle(deck)
        chunks = [lambda p=p: self.pair(*p) for p in deck[self.seed % 8::8]]
        chunks += [self.ep_a, self.ep_b, self.ep_c, self.ep_d, self.ep_e, self.ep_f, self.ep_h, self.ep_ticks]
        chunks += [lambda k=k: self.ep_reject(k) for k in REJECTIONS if k not in REJECT_CODES]
        chunks += [lambda k=k: self.ep_reject_x(k) for k in ("xshadow_flat", "xshadow_k2", "xshadow_flags")]
        chunks += [self.ep_x_own, self.ep_x_opts]
        chunks += [self.ep_x_timed, self.ep_x_cost]
        chunks += [lambda k=k: self.ep_x_after(k) for k in (("tree", "build"), ("build", "sopt"), ("sopt", "tree"))[self.seed % 3]]
        settings = [(k, v) for k, vs in OPT_VALUES.items() for v in vs] + [(K_DEBUG, b) for b in DEBUG_BITS + (0,)]
        settings += [(K_DEBUG, 4 | 2048), (K_DEBUG, 8 | 64 | 256), (K_DEBUG, 1024 | 2048 | 4), (K_DEBUG, sum(DEBUG_BITS))]
        np.random.default_rng(0x0B7).shuffle(settings)
        mine = settings[self.seed % 8::8]
        chunks += [lambda a=a: self.ep_opts(a) for a in (mine[:len(mine) // 2], mine[len(mine) // 2:])]
        scene_settings = [(k, v) for k, vs in SOPT_VALUES.items() for v in vs]
        chunks += [lambda a=a: self.ep_sopt(*a) for a in scene_settings[self.seed % 8::8]]
        chunks += [lambda a=a: self.ep_tree(a) for a in (TREES["s33"] + ("built",))[self.seed % 8::8]]
        chunks += [lambda a=a: self.ep_xf(a) for a in XF_NAMES[self.seed % 8::8]]
        chunks += [self.filler] * 8
        for i in self.rng.permutation(len(chunks)):
            chunks[int(i)]()
        return self.ops


def generate(seed):
    """The seed's operation list (deterministic)."""
    return _Gen(seed).run()


# --------------------------------------------------------------------- oracle

class World:
    """The meshes, their trees (the product's arrays and the oracle's) and the
    rejected trees: host data only."""

    def __init__(self):
        from cpp_cuda_raytracer_dev_amd import raytracer as R
        (v33, f33), variants = S.tree_variants()
        src = {"s257": S.soup(257, S.SOUP_SEED + 257), "s33": (v33, f33), "s9": S.soup(9, S.SOUP_SEED + 9),
               "s1": S.soup(1, S.SOUP_SEED + 1), "copies": S.copies(*S.COPIES), "grid": S.grid(),
               "mat": S.soup(S.LIGHT_N, S.SOUP_SEED + S.LIGHT_N)}
        self.pts, self.rad, self.leafs, self.trees, self.otrees = {}, {}, {}, {}, {}
        for name in MESHES:
            v, f = src[name]
            rad = S.material_table("materials", NTRI[name]) if name == "mat" else None
            sc = S.SynthScene(v, f, *CAMS[1], rad=rad)      # (asserts the product's builder equals the oracle's)
            self.pts[name], self.rad[name] = sc.pts, sc.rad
            assert len(sc.pts) == NTRI[name]
            self.leafs[name] = R.assemble_mesh(np.ascontiguousarray(v, F), np.ascontiguousarray(f, np.int32))[2]
            self.trees[name] = {"built": sc.nodes}
            if name == "s33":
                assert set(variants) == set(TREES["s33"]) and variants["built"].tobytes() == sc.nodes.tobytes()
                self.trees[name] = {k: variants[k] for k in TREES["s33"]}
            self.otrees[name] = {k: S.oracle_nodes(t) for k, t in self.trees[name].items()}

    def bad_tree(self, mesh, kind):
        """A node array rt_scene_set_kd must reject."""
        nodes = self.trees[mesh]["built"].copy()
        leaves = np.flatnonzero(nodes["is_leaf"] == 1)
        inner = np.flatnonzero(nodes["is_leaf"] == 0)
        if kind == "bad_dup":      # two leaves of one triangle (one leaf: a triangle out of range)
            nodes["tri_index"][leaves[-1]] = nodes["tri_index"][leaves[0]] if len(leaves) > 1 else NTRI[mesh]
        elif kind == "bad_bfs":    # a child at or before its parent
            i = inner[len(inner) // 2] if len(inner) else 0
            nodes["is_leaf"][i] = 0
            nodes["left"][i], nodes["right"][i] = i, i + 1
        elif kind == "bad_count":
            nodes = nodes[:-1].copy() if len(nodes) > 1 else np.concatenate([nodes, nodes])
        else:
            raise ValueError(kind)
        return nodes


_world = None


def world():
    global _world
    if _world is None:
        _world = World()
    return _world


class Oracle:
    """Expected frames from the C oracle, cached; the ten planes from its hit
    index by the numpy restatement's arithmetic, vectorised over the pixels."""

    def __init__(self):
        self.w = world()
        self._scenes, self._frames, self._planes, self._prep, self._rays = {}, {}, {}, {}, {}
        self._cross, self._xprep, self._xtraced = {}, {}, {}

    def _rad(self, mesh):
        return O.default_rad(NTRI[mesh]) if self.w.rad[mesh] is None else self.w.rad[mesh]

    def _scene(self, mesh, tree, ci):
        return O.Scene(self.w.pts[mesh], self._rad(mesh), self.w.otrees[mesh]["built" if tree == "-" else tree],
                       O.camera(*CAMS[ci]))

    def frame(self, spec, fresh=False):
        """-> (argb, hit, counters) of spec = (mesh, tree, ci, transform, mode, shadow)."""
        mesh, tree, ci, xf, mode, shadow = spec
        if fresh:
            sc = self._scene(mesh, tree, ci)
            try:
                return sc.render(mode, xform=np.array(xf, F), nthreads=H.ORACLE_THREADS, shadow=shadow)
            finally:
                sc.close()
        if spec not in self._frames:
            key = (mesh, tree, ci)
            if key not in self._scenes:
                self._scenes[key] = self._scene(*key)
            out = self._scenes[key].render(mode, xform=np.array(xf, F), nthreads=H.ORACLE_THREADS, shadow=shadow)
            for a in out:
                a.setflags(write=False)
            self._frames[spec] = out
        return self._frames[spec]

    def rays(self, ci):
        """The oracle's primary rays [3][w * h]."""
        if ci not in self._rays:
            import ctypes as C
            w, h = CAMS[ci]
            cam, r = O.camera(w, h), np.zeros(3, F)
            out = np.zeros((w * h, 3), F)
            for i in range(w * h):
                O.lib().orc_primary_ray(C.byref(cam), i % w, i // w, O._ptr(r))
                out[i] = r
            self._rays[ci] = out
        return self._rays[ci]

    def planes(self, spec, fresh=False):
        """-> [10, w * h] float32 bits (uint32): d, point, normal, radiance of
        the hit the oracle's frame names; d = 400 and zeros at a miss."""
        mesh, tree, ci, xf, mode, _ = spec
        key = spec[:5]
        if fresh or key not in self._planes:
            hit = self.frame(spec[:5] + (False,), fresh)[1]
            pk = (mesh, ci)
            if pk not in self._prep:
                self._prep[pk] = N.prepare(self.w.pts[mesh], None, N.camera(*CAMS[ci]))
            out = hit_planes(self._prep[pk], self.rays(ci), np.array(xf, F), mode, hit,
                             N.RAD if self.w.rad[mesh] is None else self.w.rad[mesh])
            out.setflags(write=False)
            if fresh:
                return out
            self._planes[key] = out
        return self._planes[key]

    def cross(self, layers, fresh=False):
        """The cross-shadowed frame of a composite's two layers [(spec, hit
        base)] by the numpy reference (tests/test_xshadow_cpu.cross_shadow on
        np_oracle.prepare of each spec's oracle tree and trace_object with the
        mesh's radiance table) -> (pixel indices, argb, hit, foreign, own):
        foreign[B] / own[B] the five counters of object B's shadow walks of the
        other object's pixels / of its own.  Cached per pair of specs (the
        shadow flag apart: the renders' own shadows are the passes' too);
        fresh: every CROSS_FRESH_STEP-th pixel alone, nothing cached."""
        from tests.test_xshadow_cpu import cross_shadow, trace_object
        key = tuple(spec[:5] for spec, _ in layers)
        if not fresh and key in self._cross:
            return self._cross[key]
        ci = key[0][2]
        w, h = CAMS[ci]
        cam = N.camera(w, h)
        pixels = np.arange(0, w * h, CROSS_FRESH_STEP if fresh else 1)
        Ps, traced = [], []
        for mesh, tree, _, xf, mode in key:
            assert mode == KD
            pk = (mesh, tree, ci)
            P = None if fresh else self._xprep.get(pk)
            if P is None:
                P = N.prepare(self.w.pts[mesh], N.nodes_from_array(self.w.otrees[mesh][tree]), cam)
                if not fresh:
                    self._xprep[pk] = P
            Ps.append(P)
            tk = (mesh, tree, ci, xf)
            tr = None if fresh else self._xtraced.get(tk)
            if tr is None:
                tr = trace_object(P, cam, np.array(xf, F), pixels, rad=self.w.rad[mesh])
                if not fresh:
                    self._xtraced[tk] = tr
            traced.append(tr)
        foreign, own = [[0] * 5, [0] * 5], [[0] * 5, [0] * 5]
        argb, hit, _, _ = cross_shadow(Ps, cam, [np.array(k[3], F) for k in key], pixels=pixels, traced=traced,
                                       cnt=foreign, own_cnt=own)
        assert [base for _, base in layers] == [0, NTRI[key[0][0]]]
        out = (pixels, argb, hit, np.array(foreign, np.uint64), np.array(own, np.uint64))
        for a in out:
            a.setflags(write=False)
        if not fresh:
            self._cross[key] = out
        return out

    def close(self):
        for sc in self._scenes.values():
            sc.close()
        self._scenes = {}


CROSS_FRESH_STEP = 16


def hit_planes(P, rays, X, mode, hit, rad):
    """The ten planes of the pixels' hits (hit[i] >= 0: the triangle) by the
    arithmetic of np_oracle.trace_kd's / trace_flat's accepted hit, one float32
    operation at a time over all hit pixels at once.  P: np_oracle.prepare."""
    n = len(hit)
    out = np.zeros((10, n), F)
    out[0] = F(400.0)
    idx = np.flatnonzero(hit >= 0)
    if idx.size == 0:
        return out.view(np.uint32)
    t = hit[idx]
    rmd = [rays[idx, k] for k in range(3)]
    e1 = [P["e1"][t, k] for k in range(3)]
    e2 = [P["e2"][t, k] for k in range(3)]
    nrm = [P["nrm"][t, k] for k in range(3)]
    with np.errstate(all="ignore"):
        if mode == KD:
            X = [F(x) for x in X]
            od = (X[3], X[7], X[11])
            m = [F(-c) for c in rmd]
            r = [F(F(-1) * F(F(F(X[4 * k] * m[0]) + F(X[4 * k + 1] * m[1])) + F(X[4 * k + 2] * m[2]))) for k in range(3)]
            p = N.cross(r, e2)
            pe1 = F(D(1.0) / D(N.dot(p, e1)))
            tt = [F(P["dt"][t, k] - od[k]) for k in range(3)]
            w = F(pe1 * N.dot(e2, N.cross(tt, e1)))
            pnt = [F(F(w * r[k]) + od[k]) for k in range(3)]
            a = [F(F(-1) * nrm[k]) for k in range(3)]
            nr = [F(F(F(F(a[0] * X[4 * k]) + F(a[1] * X[4 * k + 1])) + F(a[2] * X[4 * k + 2])) * F(-1)) for k in range(3)]
        else:
            p = N.cross(rmd, e2)
            pe1 = F(D(1.0) / D(N.dot(p, e1)))
            w = F(pe1 * P["dw"][t])
            pnt = [F(w * rmd[k]) for k in range(3)]
            nr = nrm
    out[0, idx] = w
    for k in range(3):
        out[1 + k, idx], out[4 + k, idx] = pnt[k], nr[k]
        out[7 + k, idx] = np.asarray(rad, F).reshape(-1, 3)[t, k] if np.ndim(rad) == 2 else F(rad[k])
    return out.view(np.uint32)


def expected(oracle, exp, fresh=False):
    """A valid render's expected (argb, hit, planes bits or None, counters):
    the oracle's frame, or the composite of its layers (tests/test_over_cpu.py)."""
    from tests.test_over_cpu import composite
    if exp.kind == "shadow":     # the pass over the camera's own buffers: the shadow frame of the render they hold
        f = oracle.frame(exp.layers[0][0], fresh)
        return f[0], f[1], None, None
    flags, over = exp.op[3], exp.op[0] == "render" and exp.op[4][0] in ("over", "xshadow")
    frames = [oracle.frame(spec, fresh) for spec, _ in exp.layers]
    cnt = np.sum([np.asarray(f[2][:5], np.uint64) for f in frames], axis=0)
    planes = [oracle.planes(spec, fresh) for spec, _ in exp.layers] if (flags & AOV or over) else None
    if over:
        argb, hit, pl = composite([(f[0], f[1], p, base) for f, p, (_, base) in zip(frames, planes, exp.layers)])
        if exp.xshadow:
            # the frame is cross_shadow's; hit index and planes are the composite's; the counters are the renders'
            # (with their own shadow walks under skip_own) plus the passes': the other object's pixels, and the
            # own ones unless skipped
            pixels, xargb, xhit, foreign, own = oracle.cross(exp.layers)
            assert (xhit == hit).all(), "the numpy composite's hit index differs from the C oracle's"
            argb = xargb.copy()
            if fresh:
                pixels, fargb, fhit, _, _ = oracle.cross(exp.layers, fresh=True)
                assert (fhit == hit[pixels]).all()
                argb[pixels] = fargb
            cnt = cnt + foreign.sum(0) + (0 if exp.xshadow[0] else own.sum(0))
        return argb, hit, pl, cnt
    return frames[0][0], frames[0][1], None if planes is None else planes[0], cnt


def unpack(packed, w, h, nranks):
    """[nranks, ..., packed pixels] -> [..., h * w]: band b (8 rows) is slot b // nranks of rank b % nranks."""
    packed = np.asarray(packed)
    lead = packed.shape[1:-1]
    rows = packed.reshape(packed.shape[:-1] + (-1, w))
    out = np.empty(lead + (h, w), packed.dtype)
    for y in range(h):
        b = y // 8
        out[..., y, :] = rows[b % nranks][..., (b // nranks) * 8 + y % 8, :]
    return out.reshape(lead + (h * w,))


# --------------------------------------------------------------------- runner

POISON = 0x7FC0DEAD


class SequenceFailure(AssertionError):
    pass


class Runner:
    """The operations on the product: two cameras and seven Trixels alive for
    the whole sequence, every render compared with the model's expectation.
    The first mismatch, device error, HIP error or unpredicted RtError ends the
    sequence (SequenceFailure); nothing is launched after it."""

    def __init__(self, oracle=None, seed=None, device=0):
        import torch
        from cpp_cuda_raytracer_dev_amd import raytracer as R
        self.torch, self.R = torch, R
        self.seed = seed
        self.oracle = oracle or Oracle()
        self.w = self.oracle.w
        self.model = Model()
        self.dev = torch.device(f"cuda:{device}")
        self.device = device
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(NSTREAMS)]
        self.trixels = {}
        for m in MESHES:
            t = R.Trixel(NTRI[m], self.w.pts[m], color_data=self.w.rad[m], device=device)
            t.set_kd_nodes(self.w.trees[m]["built"])
            self.trixels[m] = t
        self.cams = [R.Camera.default(w, h, device=device) for w, h in CAMS]
        self.objs = [None] * len(CAMS)
        self.windows = [O.Window(w * h) for w, h in CAMS]
        self.bufs = {}
        self.renders = 0
        self.passes = 0                         # deferred shadow passes among them (two per "xshadow", one per "shadow")
        self.done = []
        self.restores = [0] * len(CAMS)         # RT_OPT_ORDER_RESTORES as last read
        self.reprepared = [False] * len(CAMS)   # the camera's records follow a new object or tree
        for ci, cam in enumerate(self.cams):
            for key, value in OPT_DEFAULTS.items():
                if key in OPT_READABLE:
                    assert cam.get_option(key) == value, (key, value)

    def close(self):
        for cam, obj in zip(self.cams, self.objs):
            cam.close()
            if obj is not None and obj.motion is not None:
                obj.motion.close()
        for t in self.trixels.values():
            t.close()
        self.cams, self.trixels = [], {}

    # -- device buffers (persistent: "the same targets" are the same memory)
    def buf(self, ci, name, n, dtype, fill=POISON):
        key = (ci, name)
        if key not in self.bufs:
            self.bufs[key] = self.torch.full((n,), fill, dtype=dtype, device=self.dev)
            self.torch.cuda.synchronize()
        return self.bufs[key]

    def targets(self, ci, name, n):
        t = self.torch
        return (self.buf(ci, name + ".argb", n, t.int32), self.buf(ci, name + ".hit", n, t.int64, -9),
                self.buf(ci, name + ".planes", 10 * n, t.int32))

    def poison(self, st, *tensors):
        with self.torch.cuda.stream(st):
            for x in tensors:
                x.fill_(-9 if x.dtype == self.torch.int64 else POISON)

    @staticmethod
    def host(x):
        a = x.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a

    def untouched(self, *tensors):
        self.torch.cuda.synchronize()
        for x in tensors:
            a = x.cpu().numpy()
            assert (a == (-9 if a.dtype == np.int64 else POISON)).all(), "a rejected call wrote to its targets"

    # -- comparisons
    def same(self, what, got, want):
        if got is None or want is None:
            return
        got, want = np.asarray(got), np.asarray(want)
        if want.dtype == np.float32:
            want = want.view(np.uint32)
        want = want.reshape(got.shape)
        bad = np.flatnonzero((got != want).reshape(-1, got.shape[-1]).any(0))
        assert bad.size == 0, f"{what}: {bad.size} pixels differ, first {bad[:6]}: {got[..., bad[:3]]} vs {want[..., bad[:3]]}"

    def counters(self, exp, want, frames=1):
        from tests.test_gpu_parity import _counters_match
        ci, mode = exp.op[1], exp.op[2]
        got = self.cams[ci].counters(reset=True)
        want = [int(x) * frames for x in want]
        if mode == KD:
            _counters_match(got, want, exp.snap["kernel"])
        else:
            assert [int(got[i]) for i in (1, 2, 3)] == [want[i] for i in (1, 2, 3)], ("flat counters", got, want)

    def after_render(self, exp):
        ci, mode = exp.op[1], exp.op[2]
        from cpp_cuda_raytracer_dev_amd import _lib
        cam = self.cams[ci]
        assert cam.device_error() == 0, f"device error word {cam.device_error()}"
        if mode == KD and exp.snap["kernel"] == 3:
            assert cam.get_option(_lib.RT_OPT_RAYS_USED) in (8, 16, 32), cam.get_option(_lib.RT_OPT_RAYS_USED)
            if NTRI[self.model.cams[ci].mesh] == 1:   # the root is a leaf (the last layer's, for a composite)
                assert cam.get_option(_lib.RT_OPT_FAST_USED) == 0
        # a cost order kept from another object or tree never comes back (prepare_camera_object drops them)
        restores = cam.get_option(_lib.RT_OPT_ORDER_RESTORES)
        assert not self.reprepared[ci] or restores == self.restores[ci], \
            f"a kept cost order was restored across a new object or tree ({self.restores[ci]} -> {restores})"
        self.restores[ci], self.reprepared[ci] = restores, False
        self.renders += 1

    # -- operations
    def attach(self, ci, mesh):
        old = self.objs[ci]
        obj = self.R.Object(self.trixels[mesh])
        self.cams[ci].add_object(obj)
        self.objs[ci] = obj
        self.reprepared[ci] = True
        if old is not None and old.motion is not None:
            old.motion.close()

    def expect_error(self, exp, fn):
        from cpp_cuda_raytracer_dev_amd import _lib
        try:
            fn()
        except _lib.RtError as e:
            code = REJECT_CODES.get(exp.reject)
            assert code is None or e.code == code, f"{exp.reject}: RtError code {e.code}, documented {code}"
            return
        raise AssertionError(f"the call was accepted; the model expects it rejected ({exp.reject})")

    def shadow_pass(self, ci, *args, **kw):
        """Camera.shadow_over, which must leave what the renders' launch state
        shows (RT_OPT_ORDER_RESTORES, RT_OPT_FINE_TILES) as it was."""
        from cpp_cuda_raytracer_dev_amd import _lib
        cam = self.cams[ci]
        state = lambda: (cam.get_option(_lib.RT_OPT_ORDER_RESTORES), cam.get_option(_lib.RT_OPT_FINE_TILES))  # noqa: E731
        before = state()
        cam.shadow_over(*args, **kw)
        assert state() == before, f"the deferred shadow pass changed the renders' state: {before} -> {state()}"

    def op_xshadow(self, exp, xf, mesh):
        """The "over" composite, then the two objects' passes over the same targets."""
        from cpp_cuda_raytracer_dev_amd import _lib
        torch = self.torch
        _, ci, mode, flags, (_, mesh2, s, skip_own, first) = exp.op
        cam = self.cams[ci]
        w, h = CAMS[ci]
        n = w * h
        st = self.streams[s]
        X, ident = np.array(xf, F), np.array(IDENT, F)
        argb, hit, planes = self.targets(ci, "full", n)
        self.poison(st, argb, hit, planes)
        cam.set_aov(planes.view(torch.float32), n)
        rflags = flags | (SHADOW if skip_own else 0)
        if exp.reject:
            if exp.reject in ("flags_high", "xshadow_flat"):     # the render is the call that fails
                call = lambda: cam.render_over(argb, hit, xform=X, mode=mode, flags=rflags, hit_base=0,  # noqa: E731
                                               stream=st.cuda_stream)
            else:
                call = lambda: cam.shadow_over(argb, hit, xform=X, flags=flags, hit_base=0, skip_own=bool(skip_own),  # noqa: E731
                                               stream=st.cuda_stream)
            self.expect_error(exp, call)
            self.untouched(argb, hit, planes)
            return
        want = expected(self.oracle, exp)
        cam.clear_layers(argb, hit, stream=st.cuda_stream)
        cam.render_over(argb, hit, xform=X, mode=mode, flags=rflags, hit_base=0, stream=st.cuda_stream)
        self.restores[ci] = cam.get_option(_lib.RT_OPT_ORDER_RESTORES)   # (the first layer may restore one)
        self.attach(ci, mesh2)
        cam.render_over(argb, hit, xform=ident, mode=mode, flags=rflags, hit_base=NTRI[mesh], stream=st.cuda_stream)
        objects = ((mesh, X, 0), (mesh2, ident, NTRI[mesh]))
        for k in (first, 1 - first):
            m, Xk, base = objects[k]
            self.attach(ci, m)
            self.shadow_pass(ci, argb, hit, xform=Xk, flags=flags, hit_base=base, skip_own=bool(skip_own),
                             stream=st.cuda_stream)
        if first == 1:
            self.attach(ci, mesh2)       # the camera shows mesh2 at the identity, as "over" leaves it
        st.synchronize()
        self.same("argb", self.host(argb), want[0])
        self.same("hit", self.host(hit), want[1])
        self.same("planes", self.host(planes).reshape(10, n), want[2])
        if flags & COUNT and not exp.snap["debug"] & 16:   # (a counted walk under bit 16 stops at occluders)
            self.counters(exp, want[3])
        self.passes += 2
        self.after_render(exp)

    def op_shadow(self, exp):
        """The pass over the camera's own frame, hit index and planes."""
        from cpp_cuda_raytracer_dev_amd import _lib
        _, ci, s = exp.op
        cam = self.cams[ci]
        w, h = CAMS[ci]
        st = self.streams[s]
        cam.set_aov(None)
        frame = lambda: (np.zeros(w * h, np.uint32), np.zeros(w * h, np.int64))  # noqa: E731
        before, after = frame(), frame()
        _lib.call("rt_read_frame", cam._h, _lib.ptr(before[0]), _lib.ptr(before[1]))
        if exp.reject:
            self.expect_error(exp, lambda: cam.shadow_over(stream=st.cuda_stream))
        else:
            want = expected(self.oracle, exp)
            self.shadow_pass(ci, xform=np.array(self.model.cams[ci].xf, F), stream=st.cuda_stream)
            st.synchronize()
        _lib.call("rt_read_frame", cam._h, _lib.ptr(after[0]), _lib.ptr(after[1]))
        if exp.reject:
            assert (before[0] == after[0]).all() and (before[1] == after[1]).all(), "a rejected pass wrote a frame"
            return
        self.same("argb", after[0], want[0])
        self.same("hit", after[1], want[1])
        assert cam.device_error() == 0, f"device error word {cam.device_error()}"
        self.passes += 1
        self.renders += 1

    def op_opt(self, exp):
        from cpp_cuda_raytracer_dev_amd import _lib
        _, ci, key, value = exp.op
        cam = self.cams[ci]
        if exp.reject:
            self.expect_error(exp, lambda: cam.set_option(key, value))
            if key in OPT_RETIRED:
                self.expect_error(exp, lambda: cam.get_option(key))
        else:
            cam.set_option(key, value)
        for k in OPT_READABLE:       # the option reads back as set; a rejected value changed nothing
            assert cam.get_option(k) == self.model.cams[ci].opts[k], (k, cam.get_option(k))
        so = self.model.cams[ci].opts[K_SHADOW_ORDER]
        assert so < 0 or cam.get_option(_lib.RT_OPT_SHADOW_ORDER) == so

    def op_tree(self, exp):
        _, mesh, name = exp.op
        t = self.trixels[mesh]
        if exp.reject:
            bad = self.w.bad_tree(mesh, name)
            self.expect_error(exp, lambda: t.set_kd_nodes(bad))
        else:
            t.set_kd_nodes(self.w.trees[mesh][name])

    def op_build(self, exp):
        t = self.trixels[exp.op[1]]
        t.set_sorted_voxels(self.w.leafs[exp.op[1]], NTRI[exp.op[1]])
        assert t.create_kd(on_device=True) == 0

    def op_sopt(self, exp):
        _, mesh, key, value = exp.op
        self.trixels[mesh].set_option(key, value)
        assert self.trixels[mesh].get_option(key) == value

    def op_xf(self, exp):
        ci = exp.op[1]
        self.objs[ci].quat.rot_m = np.array(self.model.cams[ci].xf, F).reshape(3, 4)

    def op_tick(self, exp):
        ci = exp.op[1]
        self.objs[ci].key_tick(exp.op[2])
        want = np.array(self.model.cams[ci].xf, F)
        assert (self.objs[ci].quat.xform().view(np.uint32) == want.view(np.uint32)).all(), "the motion state differs"

    def op_sync(self, exp):
        s = exp.op[1]
        if s < 0:
            self.torch.cuda.synchronize()
        else:
            self.streams[s].synchronize()

    def op_render(self, exp, xf, mesh):
        """xf, mesh: the camera's transform and mesh before the model's step
        (a composite's step attaches the second layer)."""
        R, torch = self.R, self.torch
        _, ci, mode, flags, target = exp.op
        cam, obj = self.cams[ci], self.objs[ci]
        w, h = CAMS[ci]
        n = w * h
        kind = target[0]
        if kind == "xshadow":
            return self.op_xshadow(exp, xf, mesh)
        st = self.streams[target[-1]] if kind != "own" else None
        X = np.array(xf, F)
        want = None if exp.reject else expected(self.oracle, exp)
        aov = bool(flags & AOV)

        if kind == "own":
            if exp.reject:
                before = np.zeros(n, np.uint32), np.zeros(n, np.int64)
                after = np.zeros(n, np.uint32), np.zeros(n, np.int64)
                from cpp_cuda_raytracer_dev_amd import _lib
                _lib.call("rt_read_frame", cam._h, _lib.ptr(before[0]), _lib.ptr(before[1]))
                self.expect_error(exp, lambda: obj.render(cam, mode=mode, flags=flags))
                _lib.call("rt_read_frame", cam._h, _lib.ptr(after[0]), _lib.ptr(after[1]))
                assert (before[0] == after[0]).all() and (before[1] == after[1]).all(), "a rejected render wrote a frame"
                return
            if aov:
                cam.set_aov(None)
            obj.quat.rot_m = X.reshape(3, 4)
            obj.render(cam, mode=mode, flags=flags)
            cam.color_pixels()
            self.same("argb", cam.h_color, want[0])
            if flags & HIT:
                self.same("hit", cam.h_rmi, want[1])
            if aov:
                a = cam.aov()
                got = np.concatenate([a["d"][None], a["pnt"], a["norm"], a["rad"]]).view(np.uint32).reshape(10, n)
                self.same("planes", got, want[2])
        elif kind in ("into", "display", "over"):
            argb, hit, planes = self.targets(ci, "full", n)
            pf = planes.view(torch.float32)
            self.poison(st, argb, hit, planes)
            if aov or kind == "over":
                cam.set_aov(pf, n)
            hit_arg = hit if flags & HIT or kind == "over" else None
            if kind == "into":
                call = lambda: cam.render_into(argb, hit_arg, xform=X, mode=mode, flags=flags, stream=st.cuda_stream)  # noqa: E731
            elif kind == "display":
                clean = self.buf(ci, "clean", n, torch.int32, 0)     # zeros before the first frame
                call = lambda: cam.render_display(clean, argb, hit_arg, xform=X, mode=mode, flags=flags,  # noqa: E731
                                                  stream=st.cuda_stream)
            else:
                call = lambda: cam.render_over(argb, hit, xform=X, mode=mode, flags=flags, hit_base=0,  # noqa: E731
                                               stream=st.cuda_stream)
            if exp.reject:
                self.expect_error(exp, call)
                self.untouched(argb, hit, planes)
                return
            if kind == "over":
                cam.clear_layers(argb, hit, stream=st.cuda_stream)
            call()
            if kind == "over":
                from cpp_cuda_raytracer_dev_amd import _lib
                self.restores[ci] = cam.get_option(_lib.RT_OPT_ORDER_RESTORES)   # (the first layer may restore one)
                self.attach(ci, target[1])
                cam.render_over(argb, hit, xform=np.array(IDENT, F), mode=mode, flags=flags, hit_base=NTRI[mesh],
                                stream=st.cuda_stream)
            st.synchronize()
            if kind == "display":
                self.same("clean", self.host(clean), want[0])
                shown = self.windows[ci].frame(want[0], want[1])
                self.same("displayed", self.host(argb), shown)
            else:
                self.same("argb", self.host(argb), want[0])
            if hit_arg is not None:
                self.same("hit", self.host(hit), want[1])
            if aov or kind == "over":
                self.same("planes", self.host(planes).reshape(10, n), want[2])
        else:
            nranks = target[1]
            npk = R.packed_pixels(w, h, nranks)
            argb, hit, planes = self.targets(ci, f"ranks{nranks}", nranks * npk)
            frame = self.buf(ci, "frame", n, torch.int32)
            self.poison(st, argb, hit, planes, frame)
            rank = lambda r: cam.render_into(  # noqa: E731
                argb[r * npk:(r + 1) * npk], hit[r * npk:(r + 1) * npk] if flags & HIT else None, xform=X, mode=mode,
                flags=flags, tile=(nranks, r), stream=st.cuda_stream,
                aov=planes[r * 10 * npk:(r + 1) * 10 * npk].view(torch.float32) if aov else None,
                plane_stride=npk if aov else None)
            if exp.reject:
                self.expect_error(exp, lambda: rank(0))
                self.untouched(argb, hit, planes)
                return
            for r in range(nranks):
                rank(r)
            R.unpack_bands(self.device, w, h, nranks, argb, frame, stream=st.cuda_stream)
            st.synchronize()
            self.same("argb (rt_unpack_bands)", self.host(frame), want[0])
            self.same("argb", unpack(self.host(argb).reshape(nranks, npk), w, h, nranks), want[0])
            if flags & HIT:
                self.same("hit", unpack(self.host(hit).reshape(nranks, npk), w, h, nranks), want[1])
            if aov:
                self.same("planes", unpack(self.host(planes).reshape(nranks, 10, npk), w, h, nranks), want[2])
        if flags & COUNT:
            self.counters(exp, want[3])
        self.after_render(exp)

    def op_loop(self, exp, xf):
        R, torch = self.R, self.torch
        _, ci, mode, flags, nframes, inflight, nbuf, s = exp.op
        cam = self.cams[ci]
        w, h = CAMS[ci]
        st = self.streams[s]
        bufs = [self.buf(ci, f"loop{k}", w * h, torch.int32) for k in range(nbuf)]
        self.poison(st, *bufs)
        st.synchronize()
        loop = R.FrameLoop(cam, bufs, xform=np.array(xf, F), mode=mode, flags=flags, render_stream=st.cuda_stream,
                           event_every=self.renders % 3, inflight=inflight)
        if exp.reject:
            self.expect_error(exp, lambda: loop.run(nframes))
            self.untouched(*bufs)
            return
        loop.run(nframes)
        torch.cuda.synchronize()
        want = expected(self.oracle, exp)
        for k, b in enumerate(bufs):       # the last frame and the ones before it: a static scene
            self.same(f"loop buffer {k}", self.host(b), want[0])
        if flags & COUNT:
            self.counters(exp, want[3], nframes)
        self.after_render(exp)

    def step(self, op):
        c = self.model.cams[op[1]] if op[0] in ("render", "loop") else None
        xf, mesh = (c.xf, c.mesh) if c is not None else (None, None)
        exp = self.model.step(op)
        k = exp.op[0]
        if k == "attach":
            self.attach(exp.op[1], exp.op[2])
        elif k == "render":
            self.op_render(exp, xf, mesh)
        elif k == "loop":
            self.op_loop(exp, xf)
        else:
            getattr(self, "op_" + k)(exp)
        if k in ("tree", "build", "sopt") and not exp.reject:
            for ci in exp.cams:
                self.reprepared[ci] = True

    def run(self, ops):
        ops = [_norm(op) for op in ops]
        for i, op in enumerate(ops):
            try:
                self.step(op)
            except Exception as e:  # a mismatch, a HIP error, an RtError the model did not predict: stop here
                raise SequenceFailure(
                    f"seed {self.seed}, step {i} {op!r}: {type(e).__name__}: {e}\n"
                    f"replay with tests.seq.replay({ops[:i + 1]!r})") from e
            self.done.append(op)


def replay(ops, seed=None, oracle=None):
    """Run an operation list on fresh cameras and scenes (needs a GPU)."""
    r = Runner(oracle, seed)
    try:
        r.run(ops)
    finally:
        r.close()
    return r
