"""The numpy reference of the light list (rt_light_over, rt_shade_lights):
deferred shading and shadows of a composite for up to eight lights, built on
oracle/np_oracle.py's walk and arithmetic, tests/test_xshadow_cpu.py's
trace_object and tests/test_over_cpu.py's composite.  The GPU tests compare
with ``lit_composite``; nothing here calls the library."""
import numpy as np

from oracle import np_oracle as N
from oracle.np_oracle import SHADOW_SCALE, D, F, _mt_accept, _walk, dev_normalize, dot, pow5, to_u8
from tests.test_over_cpu import composite
from tests.test_xshadow_cpu import trace_object

LIGHTS_MAX = 8
DEFAULT_LIGHTS = ((2.0, 2.0, 2.0, 1.0),)


def as_lights(lights):
    a = np.asarray(lights, F).reshape(-1, 4)
    assert 1 <= len(a) <= LIGHTS_MAX
    return a


def shadow_from(S, rmi, d, ray, L, cnt=None):
    """np_oracle.trace_shadow with the light L = (Lx, Ly, Lz) for the literal
    (2,2,2): the segment from L to H = d*r - od, walked from the light with
    the ray offset -L; True if occluded."""
    r, od = ray
    sv = [F(F(F(d * r[k]) - od[k]) - F(L[k])) for k in range(3)]
    L2 = F(F(F(sv[0] * sv[0]) + F(sv[1] * sv[1])) + F(sv[2] * sv[2]))
    lmax = F(F(np.sqrt(D(L2))) * SHADOW_SCALE)
    s = dev_normalize(*sv)
    hit = [False]

    def leaf(t, u, v, w):
        if t != rmi and _mt_accept(u, v, w, lmax):
            if cnt is not None:
                cnt[2] += 1
            hit[0] = True

    _walk(S, list(s), (F(-F(L[0])), F(-F(L[1])), F(-F(L[2]))), leaf, lim=lmax, cnt=cnt)
    return hit[0]


def light_terms(pnt, nrm, rmd, L):
    """(diff, spec) of np_oracle.phong with L - pnt for 2 - pnt."""
    sd = dev_normalize(F(F(L[0]) - pnt[0]), F(F(L[1]) - pnt[1]), F(F(L[2]) - pnt[2]))
    dn = dot(sd, (nrm[0], nrm[0], nrm[2]))
    r = [F(F(sd[k] - F(F(F(2) * dn) * nrm[k])) * rmd[k]) for k in range(3)]
    diff = F(0.6 * D(abs(dn)))
    spec = F(D(pow5(abs(F(F(r[0] + r[1]) + r[2])))) * 0.3)
    return diff, spec


def normalise(c):
    mx = np.fmax(np.fmax(c[0], c[1]), c[2])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = [to_u8(F(F(c[k] / mx) * F(255))) for k in range(3)]
    return (q[0] << 16) | (q[1] << 8) | q[2]


def phong_lights(pnt, nrm, rmd, rad, lights, occ):
    """The colour of a hit pixel: from c = 0, for each light l in index order
    whose bit in occ is clear, c_k = c_k + I_l * (rad_k * diff + spec); then
    one normalisation by the largest channel."""
    c = [F(0), F(0), F(0)]
    with np.errstate(all="ignore"):
        for l, L in enumerate(as_lights(lights)):
            if (occ >> l) & 1:
                continue
            diff, spec = light_terms(pnt, nrm, rmd, L)
            c = [F(c[k] + F(L[3] * F(F(F(rad[k]) * diff) + spec))) for k in range(3)]
        return normalise(c)


def lit_composite(S, cam, xforms, lights, pixels=None, traced=None, depth=None, shadow=shadow_from, shade=phong_lights,
                  foreign_own=False):
    """The composite of one object per transform in `xforms` lit by `lights`
    ([n, 4]: Lx, Ly, Lz, I), at the pixel indices `pixels` (all by default).

    S, traced, depth: as tests.test_xshadow_cpu.cross_shadow's.  Object B
    occludes light l at a hit pixel p iff shadow_from(S_B, rmi, d, B's ray of
    p, L_l), with rmi = hit[p] - base_B on B's own pixels and -1 elsewhere;
    the pixel's mask holds bit l when some object does; its colour is
    phong_lights of planes 1-9 and p's primary ray.
    shadow / shade / foreign_own: the restated faults of the CPU tests replace
    the rules here (foreign_own: the pixel's triangle index, within its
    owner, is excluded from every object's walk, not from its owner's alone).
    -> (argb u32 [m], hit i64 [m], planes u32 bits [10, m], mask u8 [m], info)
    with info = {"owner": i64 [m], "by": bool [nobj, nlights, m], "cnt":
    [nobj][nlights] lists of five counters (every tested pixel's full walk)}."""
    lights = as_lights(lights)
    Ss = S if isinstance(S, list) else [S] * len(xforms)
    n = cam["w"] * cam["h"]
    pixels = np.arange(n) if pixels is None else np.asarray(pixels)
    if traced is None:
        traced = [trace_object(Ss[k], cam, xforms[k], pixels) for k in range(len(xforms))]
    bases = np.concatenate([[0], np.cumsum([len(s["e1"]) for s in Ss])]).astype(np.int64)
    argb, hit, planes = composite([(t[0], t[1], t[2], bases[k]) for k, t in enumerate(traced)])
    argb = argb.copy()
    m = len(pixels)
    owner = np.full(m, -1, np.int64)
    for k in range(len(xforms)):
        owner[(hit >= bases[k]) & (hit < bases[k + 1])] = k
    by = np.zeros((len(xforms), len(lights), m), bool)
    cnt = [[[0, 0, 0, 0, 0] for _ in lights] for _ in xforms]
    pl = planes.view(F)
    w = cam["w"]
    with np.errstate(all="ignore"):
        for j in np.nonzero(hit >= 0)[0]:
            d = pl[0][j] if depth is None or int(j) not in depth else F(depth[int(j)])
            for B in range(len(xforms)):
                rmi = int(hit[j] - bases[B]) if owner[j] == B else (int(hit[j] - bases[owner[j]]) if foreign_own else -1)
                for l, L in enumerate(lights):
                    by[B, l, j] = shadow(Ss[B], rmi, d, traced[B][3][j], L, cnt=cnt[B][l])
    mask = np.zeros(m, np.uint8)
    for l in range(len(lights)):
        mask |= (by[:, l].any(0).astype(np.uint8) << l).astype(np.uint8)
    for j in np.nonzero(hit >= 0)[0]:
        iy, ix = divmod(int(pixels[j]), w)
        rmd = N.primary_ray(cam, ix, iy)
        argb[j] = shade(pl[1:4, j], pl[4:7, j], rmd, pl[7:10, j], lights, int(mask[j]))
    return argb, hit, planes, mask, {"owner": owner, "by": by, "cnt": cnt}


def light_class_counts(info, l):
    """tests.test_xshadow_cpu.class_counts of a two-object frame for light l."""
    o, by = info["owner"], info["by"][:, l]
    return (int(((o == 1) & by[0] & ~by[1]).sum()), int(((o == 1) & by[0] & by[1]).sum()),
            int(((o == 0) & by[1] & ~by[0]).sum()), int(((o == 0) & by[1] & by[0]).sum()))


def summed_counters(info, B):
    """The five counters of object B's counted pass: its per-light walks summed."""
    return [sum(c[k] for c in info["cnt"][B]) for k in range(5)]
