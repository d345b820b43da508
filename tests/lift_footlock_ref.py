"""mp_lift_footlock's rule (include/manipose_hip.h) stated in numpy float64, the scenes its tests share, and their bounds.

The statement works on the float32 inputs the kernel gets and follows the header step by step, one (frame, foot) at a time, with the header's
operations in the header's order; a run's sum is numpy's, in numpy's order (the kernel adds a tree inside every 64 frames).  Beside the kernel's
outputs it returns what the kernel does not: per sequence the scale L - the largest |coordinate| of a leg joint in a good, finite frame - and the
DECISION MARGINS of every row, the distance of each branch of the rule from its border:
  tie     an anchor's coordinate from the middle of two float32 neighbours (the anchor is rounded to float32 once), in units of how far two fp64
          evaluations of it can lie apart: (run length + 16) u times the largest |term| of the coordinate's sum, times L with a floor; only of
          anchors whose sum is not exact in every order (the sums of float32 numbers of one size are: inf says every compared sum was);
  reach   D from Dmin and from Dmax, over l1 + l2 (the clamp's two borders; a leg that is clamped is as far outside as one that is not is inside);
  pole    |b| / l1 of a leg that keeps its own pole (the smallest) and of one that takes an axis (the largest);
  floor   |(n . t) - offset| of a frame outside runs in a sequence with a floor, over L;
  bend    y / l1 of a re-posed leg without a reach clamp: the knee's distance from the hip-ankle line, where the IK is ill-conditioned near 0;
  weight  the smallest weight that is > 0 (they are 1 - j / L for integers j < L <= 33: 1 / 33 at the least, asked to be above 1 / 34);
  tiny    l1, l2 and D over 1e-12.
With ``jitter`` = (generator, delta) every target t of step C and the lengths l1, l2 and D of step D are disturbed by delta, relative to L and to
themselves: ``amplification`` measures from it how far an error of the intermediate values travels into the outputs."""
import functools

import numpy as np

U = 2.0 ** -53
TIE_MIN = 4.0         # an anchor coordinate's distance from a float32 rounding tie, in units of the distance two summation orders can lie apart
REACH_MIN = 1e-6      # |D - Dmin|, |D - Dmax| over l1 + l2 of every compared leg
POLE_MIN, POLE_MAX = 1e-4, 1e-12      # |b| / l1 of a leg that keeps its pole is above the first, of one that takes an axis below the second (rule: 1e-9)
FLOOR_MIN = 1e-7      # |(n . t) - offset| / L of every compared frame outside runs
BEND_MIN = 1e-3       # y / l1 of every leg re-posed without a reach clamp
TINY_MIN = 1e6        # l1, l2, D over 1e-12 of every compared leg that has a length (a leg without one is exactly 0)
H36M_LEGS = ((1, 2, 3), (4, 5, 6))
FLOATS = ("out", "target", "moved")


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _norm(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def footlock(points, contact, off=None, valid=None, legs=H36M_LEGS, floor=None, blend=5, stretch=1.0, jitter=None):
    """the rule on points (Ntot, J, C) float32, contact (Ntot, nf) -> a dict under the kernel's names (out float32; target, moved float64 holding
    float32 values), plus ``scale`` (S), ``margin`` (a dict, see above) and ``clamped`` / ``posed`` (Ntot, nf) bool.  floor = (normal (S, 3), offset
    (S), ok (S)) or None"""
    points = np.asarray(points)
    assert points.dtype == np.float32 and points.ndim == 3
    ntot, J, _ = points.shape
    off = np.array([0, ntot]) if off is None else np.asarray(off)
    S, nf, B = len(off) - 1, len(legs), int(blend)
    stretch = float(np.float32(stretch))
    x = points[..., :3].astype(np.float64)
    good = np.ones(ntot, bool) if valid is None else np.asarray(valid) != 0
    finite = np.isfinite(x).all(axis=2)
    out = points.copy()
    res = dict(out=out, run=np.zeros((ntot, nf), np.int32), target=np.zeros((ntot, nf, 3)), moved=np.zeros((ntot, nf)), flags=np.zeros((ntot, nf), np.uint8),
               runs=np.zeros((S, nf), np.int32), scale=np.zeros(S), clamped=np.zeros((ntot, nf), bool), posed=np.zeros((ntot, nf), bool),
               out64=np.where(np.isfinite(x), x, 0.0), target64=np.zeros((ntot, nf, 3)), moved64=np.zeros((ntot, nf)))      # before the rounding to float32
    mg = dict(tie=np.inf, reach=np.inf, pole_own=np.inf, pole_axis=0.0, floor=np.inf, bend=np.inf, weight=np.inf, tiny=np.inf)
    for s in range(S):
        f0 = min(max(int(off[s]), 0), ntot)
        f1 = min(max(int(off[s + 1]), f0), ntot)
        joints = sorted(j for leg in legs for j in leg)
        seen = good[f0:f1, None] & finite[f0:f1][:, joints]
        L = float(np.abs(x[f0:f1][:, joints][seen]).max()) if seen.any() else 0.0
        res["scale"][s] = L
        has = floor is not None and bool(int(floor[2][s]) & 1)
        if has:
            n, o = np.asarray(floor[0][s], np.float32).astype(np.float64), float(np.float32(floor[1][s]))
            has = bool(np.isfinite(n).all() and np.isfinite(o))
        anchor = np.zeros((ntot, nf, 3))
        for k, (hj, kj, aj) in enumerate(legs):
            # A: lockable frames and runs
            lock = np.zeros(ntot, bool)
            lock[f0:f1] = good[f0:f1] & (np.asarray(contact)[f0:f1, k] != 0) & finite[f0:f1, hj] & finite[f0:f1, kj] & finite[f0:f1, aj]
            f = f0
            while f < f1:
                if not lock[f]:
                    f += 1
                    continue
                e = f
                while e + 1 < f1 and lock[e + 1]:
                    e += 1
                n_run = e - f + 1
                # B: the anchor
                a = x[f:e + 1, aj].sum(axis=0) / float(n_run)
                if has:
                    a = a - (_dot(n, a) - o) * n
                a32 = _f32(a)
                # Two fp64 evaluations of the sum agree to the bit where it is EXACT in every order: the terms are multiples of q, their smallest
                # float32 spacing, and sum |x| < 2^53 q (the division and the projection are then the same operations on the same bits).  Else they
                # lie at most (n_run + 16) u times the largest |term| apart (times L with a floor: 16 u L for the projection), and the margin is a's
                # distance from the middle of a32 and its neighbour on a's side, in those.
                terms = x[f:e + 1, aj]
                q = np.where(terms != 0, np.spacing(np.abs(terms).astype(np.float32)).astype(np.float64), np.inf).min(axis=0)
                exact = np.abs(terms).sum(axis=0) < 2.0 ** 53 * q
                reach = (n_run + 16) * U * (np.full(3, L) if has else np.abs(terms).max(axis=0))
                half = np.abs(np.abs(a - a32) - 0.5 * ulp32(a32))
                if not exact.all():
                    mg["tie"] = min(mg["tie"], float((half[~exact] / reach[~exact]).min()))
                res["run"][f:e + 1, k] = n_run
                anchor[f:e + 1, k] = a32
                res["runs"][s, k] += 1
                f = e + 1
        for k, (hj, kj, aj) in enumerate(legs):
            run = res["run"][:, k]
            for f in range(f0, f1):
                if not (good[f] and finite[f, hj] and finite[f, kj] and finite[f, aj]):
                    continue
                h, kn, a = x[f, hj], x[f, kj], x[f, aj]
                flags = 0
                # C: the target
                if run[f] > 0:
                    t, flags = anchor[f, k].copy(), 1
                else:
                    t = a.copy()
                    fa = next((g for g in range(f - 1, max(f0, f - B) - 1, -1) if run[g] > 0), None)
                    fb = next((g for g in range(f + 1, min(f1 - 1, f + B) + 1) if run[g] > 0), None)
                    Lr = min(B + 1, fb - fa) if fa is not None and fb is not None else B + 1
                    for g, dist in ((fa, None if fa is None else f - fa), (fb, None if fb is None else fb - f)):
                        if g is None:
                            continue
                        w = 1.0 - float(dist) / float(Lr)
                        if w > 0.0:
                            sw = (w * w) * (3.0 - 2.0 * w)
                            t = t + sw * (anchor[g, k] - x[g, aj])
                            flags |= 2
                            mg["weight"] = min(mg["weight"], w)
                    if has:
                        hh = _dot(n, t) - o
                        if L > 0:
                            mg["floor"] = min(mg["floor"], abs(hh) / L)
                        if hh < 0.0:
                            t = t - hh * n
                            flags |= 8
                if jitter is not None:
                    t = t + jitter[1] * L * jitter[0].standard_normal(3)
                # D: the leg
                l1, l2 = _norm(kn - h), _norm(a - kn)
                d = t - h
                D = _norm(d)
                if jitter is not None:
                    l1, l2, D = (v * (1.0 + jitter[1] * jitter[0].standard_normal()) for v in (l1, l2, D))
                if l1 < 1e-12 or l2 < 1e-12 or D < 1e-12:
                    res["flags"][f, k] = 32
                    mg["tiny"] = min(mg["tiny"], min(v / 1e-12 if v > 0 else np.inf for v in (l1, l2, D)))
                    continue
                mg["tiny"] = min(mg["tiny"], min(l1, l2, D) / 1e-12)
                Dmin = abs(l1 - l2)
                Dmax = max(stretch * (l1 + l2), Dmin)
                u = d / D
                Dc = D
                if D > Dmax:
                    Dc, flags = Dmax, flags | 4
                elif D < Dmin:
                    Dc, flags = Dmin, flags | 4
                mg["reach"] = min(mg["reach"], abs(D - Dmax) / (l1 + l2), abs(D - Dmin) / (l1 + l2) if Dmin > 0 else np.inf)
                if flags & 4:
                    t = h + u * Dc
                res["flags"][f, k], res["target"][f, k], res["clamped"][f, k], res["target64"][f, k] = flags, _f32(t), bool(flags & 4), t
                if jitter is None and (t == a).all():
                    continue                                              # the foot is where it belongs: the leg keeps its bits
                kh = kn - h
                b = kh - _dot(kh, u) * u
                bn = _norm(b)
                if bn < 1e-9 * l1:
                    mg["pole_axis"] = max(mg["pole_axis"], bn / l1)
                    i = int(np.argmin(np.abs(u)))                         # (the first of the smallest)
                    e = np.zeros(3)
                    e[i] = 1.0
                    b = e - u[i] * u
                    bn = _norm(b)
                    res["flags"][f, k] |= 16
                else:
                    mg["pole_own"] = min(mg["pole_own"], bn / l1)
                xx = ((Dc * Dc + l1 * l1) - l2 * l2) / (2.0 * Dc)
                yy = np.sqrt(max(0.0, l1 * l1 - xx * xx))
                if not flags & 4:
                    mg["bend"] = min(mg["bend"], yy / l1)
                knee = (h + xx * u) + yy * (b / bn)
                out[f, kj, :3] = knee.astype(np.float32)
                out[f, aj, :3] = t.astype(np.float32)
                res["moved"][f, k] = float(np.float32(_norm(_f32(t) - a)))
                res["out64"][f, kj], res["out64"][f, aj], res["moved64"][f, k] = knee, t, _norm(t - a)
                res["posed"][f, k] = True
    res["margin"] = mg
    return res


def margins_hold(mg):
    """every decision of the rule was taken away from its border (the device test and the host test both ask this of every compared case)"""
    return (mg["tie"] >= TIE_MIN and mg["reach"] >= REACH_MIN and mg["pole_own"] >= POLE_MIN and mg["pole_axis"] <= POLE_MAX and mg["floor"] >= FLOOR_MIN
            and mg["bend"] >= BEND_MIN and mg["weight"] >= 1.0 / 34.0 and mg["tiny"] >= TINY_MIN)


def frame_scale(want, off):
    """scale (S) spread over the frames (Ntot,); 1e-30 for a frame that no sequence holds"""
    out = np.full(len(want["run"]), 1e-30)
    for s in range(len(off) - 1):
        out[int(off[s]):int(off[s + 1])] = max(want["scale"][s], 1e-30)
    return out


def bound(key, want, off):
    """the largest |device - statement| of a float output: one float32 ulp of max(|want|, L)"""
    L = frame_scale(want, off)
    w = np.asarray(want[key], np.float64)[..., :3] if key == "out" else np.asarray(want[key], np.float64)
    w = np.abs(np.where(np.isfinite(w), w, 0.0))                          # (out carries the input's NaN where nobody wrote)
    return ulp32(np.maximum(w, L.reshape((-1,) + (1,) * (w.ndim - 1))))


def amplification(inp, want, draws=2, delta=1e-9, seed=0):
    """max over the float outputs and ``draws`` disturbed runs of |disturbed - want| / L / delta over the frames a sequence holds: how far a relative
    error delta of step C's target and step D's lengths travels.  (Sampled, not a worst case: the bound leaves it a factor.)"""
    g = np.random.default_rng(seed)
    worst = 0.0
    L = frame_scale(want, inp["off"])
    for _ in range(draws):
        got = footlock(inp["points"], inp["contact"], inp["off"], inp["valid"], **inp["opts"], jitter=(g, delta))
        assert np.array_equal(got["run"], want["run"]) and np.array_equal(got["flags"] & 47, want["flags"] & 47)
        for key in FLOATS:                                                # (held against each other before the rounding to float32)
            err = np.abs(got[key + "64"] - want[key + "64"])
            worst = max(worst, float((err / L.reshape((-1,) + (1,) * (err.ndim - 1))).max()) / delta)
    return worst


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def _runs_to_contact(n, runs):
    c = np.zeros(n, np.uint8)
    for a, b in runs:
        c[a:b + 1] = 1
    return c


def scene(seed, lens, contacts, J=17, C=3, legs=H36M_LEGS, lead=2, tail=3, noise=0.003, drift=0.002):
    """Sequences laid end to end after ``lead`` frames that no sequence holds, ``tail`` more behind.  contacts[s][k] = [(first, last), ...]: the frames
    of sequence s in which foot k is in contact, counted from the sequence's first.  Every leg hangs under a hip that sways; the ankle swings on a
    curve and, while in contact, stays near where it was at the contact's first frame, drifting by ``drift`` a frame under ``noise``; the knee is
    bent forward.  The whole scene is turned and moved at random.  -> points (Ntot, J, C) float32, contact (Ntot, nf) uint8, off (S + 1)"""
    from lift_ground_ref import _rotation
    g = np.random.default_rng(seed)
    nf = len(legs)
    off = lead + np.concatenate([[0], np.cumsum(lens)])
    ntot = int(off[-1]) + tail
    pos = g.standard_normal((ntot, J, 3)) * 0.3 + [0, 0, 1.0]
    contact = np.zeros((ntot, nf), np.uint8)
    for s, n in enumerate(lens):
        t = np.arange(n)
        for k, (hj, kj, aj) in enumerate(legs):
            c = _runs_to_contact(n, contacts[s][k]) if n else np.zeros(0, np.uint8)
            contact[off[s]:off[s + 1], k] = c
            ph = g.uniform(0, 6.28)
            hip = np.stack([0.02 * t + 0.03 * np.sin(0.2 * t + ph), 0.12 * (k - 0.5 * (nf - 1)) + 0.02 * np.cos(0.13 * t), 0.9 + 0.02 * np.sin(0.3 * t + ph)], 1)
            ank = hip + np.stack([0.2 * np.sin(0.3 * t + ph), 0.03 * np.cos(0.21 * t), -0.78 + 0.06 * np.cos(0.3 * t + ph)], 1)
            for a, b in contacts[s][k] if n else ():
                ank[a:b + 1] = ank[a] + drift * (t[a:b + 1] - a)[:, None] * np.array([1.0, 0.3, 0.0]) + [0, 0, -0.01]
            knee = 0.5 * (hip + ank) + [0.17, 0.01 * k, 0.02]
            for j, v in ((hj, hip), (kj, knee), (aj, ank)):
                pos[off[s]:off[s + 1], j] = v + noise * g.standard_normal(v.shape)
    R, T = _rotation(g), g.uniform(-3, 3, 3)
    pts = np.zeros((ntot, J, C), np.float32)
    pts[..., :3] = (pos @ R.T + T).astype(np.float32)
    if C == 4:
        pts[..., 3] = g.random((ntot, J)).astype(np.float32)
    return dict(points=pts, contact=contact, off=off.astype(np.int64), up=R[:, 2].copy(), origin=T)


def _floor_of(sc, legs, ok, lift=0.0):
    """a floor per sequence: the scene's own up, through the lowest ankle of the sequence raised by ``lift`` (some swing feet end below it)"""
    S = len(sc["off"]) - 1
    normal = np.tile(sc["up"].astype(np.float32), (S, 1))
    offset = np.zeros(S, np.float32)
    for s in range(S):
        a = sc["points"][sc["off"][s]:sc["off"][s + 1]][:, [leg[2] for leg in legs], :3].astype(np.float64)
        a = a[np.isfinite(a).all(axis=2)]
        offset[s] = np.float32((a @ normal[s].astype(np.float64)).min() + lift) if len(a) else 0
    return normal, offset, np.asarray(ok, np.uint8)


def _case(tag, sc, valid=None, floor=None, **opts):
    o = dict(dict(legs=H36M_LEGS, blend=5, stretch=1.0), **opts)
    inp = dict(points=sc["points"], contact=sc["contact"], off=sc["off"], valid=valid, opts=dict(o, floor=floor))
    return tag, inp, footlock(sc["points"], sc["contact"], sc["off"], valid, floor=floor, **o)


FOUR_LEGS = ((1, 2, 3), (4, 5, 6), (11, 12, 13), (14, 15, 16))


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, inputs, the statement's outputs).  The shapes are the smallest at which the kernels can still go wrong; the comments name what each
    sequence is there for.  B = blend."""
    B = 5
    # sequences of 1, 2 and 3 frames, an empty one between two others, 130 frames (three blocks of 64), 40 and 70 frames; two frames before the first
    # sequence and three behind the last that no sequence holds
    lens = (1, 2, 3, 0, 130, 40, 70)
    contacts = (
        ([(0, 0)], []),                                                   # a run of one frame that is the whole sequence
        ([(0, 1)], [(1, 1)]),                                             # the whole sequence; a run at the last frame
        ([(0, 0), (2, 2)], [(1, 1)]),                                     # runs at the first and the last frame, a gap of 1; a run of one frame
        ([], []),
        # foot 0: a run at the first frame, 60..70 across the block border, a gap of 1, a run of one frame, a run at the last frame
        # foot 1: gaps of B and B + 2 frames, and 64..127: the second block exactly
        ([(0, 3), (60, 70), (72, 72), (126, 129)], [(10, 20), (21 + B, 30), (31 + B + 2, 45), (64, 127)]),
        ([(0, 39)], [(0, 39)]),                                           # valid holes and a NaN knee split these runs (below)
        ([(0, 69)], []),                                                  # the whole sequence, across a block border
    )
    a = scene(11, lens, contacts)
    valid = np.ones(len(a["points"]), np.uint8)
    o5 = int(a["off"][5])
    valid[[o5 + 20, o5 + 21, o5 + 30]] = 0                                  # holes inside a run: they split it
    a["points"][o5 + 20] = np.nan                                           # (a frame that is not good is never read)
    a["points"][o5 + 10, 5, 1] = np.nan                                     # a NaN knee in a contact frame of foot 1: the run splits, the foot is left alone
    a["points"][int(a["off"][4]) + 50, 2, 0] = np.inf                       # ... and one outside every run
    a["points"][:2] = np.nan                                                # frames that no sequence holds are never read either
    fl = _floor_of(a, H36M_LEGS, ok=(3, 3, 1, 3, 1, 0, 3), lift=0.03)        # sequence 5 has no plane: floor off there; swing feet below the floor in 4
    b = scene(12, (7, 66), (([(2, 4)],), ([(0, 0), (3, 63), (65, 65)],)), J=5, C=4, legs=((1, 2, 3),), lead=0, tail=0)
    c = scene(13, (130, 50), (([(0, 129)], [(5, 9), (40, 100)], [(63, 64)], [(127, 128)]), ([(0, 10)], [], [(20, 49)], [(25, 25)])), C=4, legs=FOUR_LEGS,
              lead=1, tail=0, drift=0.004)
    d = scene(14, (90,), (([(5, 30), (50, 52)], [(0, 89)]),), lead=0, tail=0, drift=0.015)      # a foot that slides 0.4 m in its run: beyond reach
    return (
        _case("J=17 C=3, lengths 1 2 3 0 130 40 70, holes, NaN, floor", a, valid, fl, blend=B),
        _case("the same without a floor, stretch 0.95", a, valid, None, blend=B, stretch=0.95),
        _case("J=5 C=4, one foot, B=0", b, None, None, legs=((1, 2, 3),), blend=0),
        _case("four feet, C=4, B=32, floor", c, None, _floor_of(c, FOUR_LEGS, ok=(1, 3), lift=0.02), legs=FOUR_LEGS, blend=32),
        _case("a run that slides beyond reach, B=8", d, None, None, blend=8),
    )


# ---- constructed scenes: dyadic numbers, on which kernel and statement are exact --------------------------------------------------------------
def dyadic_scene(frames=24, slide=0.0, contact=(4, 19)):
    """A leg (1, 2, 3) standing at dyadic positions - hip (0, 0, 1), knee (1/4, 0, 1/2), ankle (0, 0, 0) - whose ankle slides by ``slide`` per frame
    along y; the other leg (4, 5, 6) mirrored at x = 2 and still.  Foot 0 is in contact in contact[0]..contact[1], foot 1 never."""
    pts = np.zeros((frames, 17, 3), np.float32)
    pts[:, :, 0] = 0.5 * np.arange(17)[None]
    pts[:, :, 2] = 1.5
    pts[:, 1], pts[:, 2], pts[:, 3] = (0, 0, 1), (0.25, 0, 0.5), (0, 0, 0)
    pts[:, 4], pts[:, 5], pts[:, 6] = (2, 0, 1), (2.25, 0, 0.5), (2, 0, 0)
    pts[:, 3, 1] = np.float32(slide) * np.arange(frames, dtype=np.float32)
    c = np.zeros((frames, 2), np.uint8)
    if contact is not None:
        c[contact[0]:contact[1] + 1, 0] = 1
    return pts, c


def straight_leg_scene():
    """Two frames in contact; the leg (1, 2, 3) hangs straight down the z axis: hip (0, 0, 1), ankle (0, 0, 0) then (0, 0, 1/4), the knee half way.
    The anchor is (0, 0, 1/8): frame 0 is pulled up by 1/8 - within reach, the knee has no side, the pole comes from the x axis (u = -z: x is the
    first of its smallest components) -, frame 1 is pushed down by 1/8 - D = 7/8 beyond l1 + l2 = 3/4: clamped, the leg stays straight."""
    pts = np.zeros((2, 17, 3), np.float32)
    pts[:, :, 0] = 0.5 * np.arange(17)[None] + 4.0
    pts[:, 1] = (0, 0, 1)
    pts[0, 2], pts[0, 3] = (0, 0, 0.5), (0, 0, 0)
    pts[1, 2], pts[1, 3] = (0, 0, 0.625), (0, 0, 0.25)
    c = np.zeros((2, 2), np.uint8)
    c[:, 0] = 1
    return pts, c


# ---- recovery ----------------------------------------------------------------------------------------------------------------------------------
def recovery_scene(seed, frames=300, noise=0.005, drifting=0.1):
    """lift_ground_ref's walker with legs under it: known plants (the stance ankle exactly still on the floor), hips 0.9 m above the feet's centre, the
    knees bent forward; ``noise`` on every joint, and in ``drifting`` of the stance frames, in one stretch per foot, the ankle slides off by 2 mm a frame.
    -> points float32, contact = the true stance, truth (frames, 2, 3): the clean ankles, normal, offset: the true floor"""
    import lift_ground_ref as gref
    w = gref.walker(2000 + seed, frames, noise=0.0, move=False)
    g = np.random.default_rng(3000 + seed)
    foot = w["truth"].copy()                                               # (move=False: the floor is z = 0)
    pos = w["points"][..., :3].astype(np.float64)
    centre = foot.mean(axis=1) * [1, 1, 0]
    dirty = foot.copy()
    for k in range(2):
        st = np.nonzero(w["stance"][:, k])[0]
        n = max(int(round(drifting * len(st))), 1)
        a = int(g.integers(0, len(st) - n))
        for i, f in enumerate(st[a:a + n]):
            dirty[f, k] += 0.002 * (i + 1) * np.array([0.8, 0.6, 0.0])
        hip = centre + [0.0, 0.1 * (2 * k - 1), 0.9]
        pos[:, 1 + 3 * k], pos[:, 3 + 3 * k] = hip, dirty[:, k]
        mid, dist = 0.5 * (hip + dirty[:, k]), np.linalg.norm(dirty[:, k] - hip, axis=1)
        pos[:, 2 + 3 * k] = mid + np.sqrt(np.maximum(0.52 ** 2 - (0.5 * dist) ** 2, 0.0))[:, None] * np.array([1.0, 0.0, 0.0])
    pts = (pos + noise * g.standard_normal(pos.shape)).astype(np.float32)
    return dict(points=pts, contact=w["stance"].astype(np.uint8), truth=foot, normal=np.array([0.0, 0.0, 1.0]), offset=0.0, stance=w["stance"])


def skate(points, contact, off, ankles, floor=None, valid=None):
    """the foot skate of points over the contact pairs (both frames good, the ankle finite), as lock_feet reports it -> (skate (S), pairs (S))"""
    contact = (np.asarray(contact) != 0) & np.isfinite(points[:, list(ankles), :3]).all(axis=2)
    if valid is not None:
        contact = contact & (np.asarray(valid) != 0)[:, None]
    S = len(off) - 1
    sk, pairs = np.zeros(S), np.zeros(S, np.int64)
    for s in range(S):
        p, c = points[off[s]:off[s + 1]][:, list(ankles), :3].astype(np.float64), contact[off[s]:off[s + 1]] != 0
        if len(p) < 2:
            continue
        pair = c[:-1] & c[1:]
        d = p[1:] - p[:-1]
        if floor is not None and int(floor[2][s]) & 1:
            n = np.asarray(floor[0][s], np.float64)
            d = d - (d @ n)[..., None] * n
        pairs[s] = pair.sum()
        with np.errstate(invalid="ignore"):
            sk[s] = np.linalg.norm(d, axis=2)[pair].sum() / pairs[s] if pairs[s] else 0.0
    return sk, pairs
