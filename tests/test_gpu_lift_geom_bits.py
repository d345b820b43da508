"""The multi-view lifting kernels share their geometry (manipose_amd/csrc/lift_geom.h: rotation, camera model, the 3x3 and 4x4 solves), so a
change there reaches every one of them at once.  tests/golden/lift_geom_bits.npz holds the raw outputs of the commit BEFORE that header existed,
when every kernel file carried its own copy, recorded on gfx950 with this toolchain by tools/gen_golden_lift_geom_bits.py on the scenes the
statement tests use.  Every entry point must reproduce those bytes: a moved parenthesis, a changed operand order or a fused multiply-add where
there was none shows here, which the tolerance tests against float64 would not notice.  (mp_lift_place and mp_lift_place_refine are held the same
way by tests/golden/lift_place_bits.npz: test_gpu_lift_refine.py.)

One record_*() per entry point regenerates the scenes from their seeds and returns {name: array}; the generator stores exactly these and the
tests compare exactly these, so the two cannot drift apart."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lift_align_ref
import lift_bundle_ref
import lift_fuse_path_ref
import lift_fuse_ref
import lift_score_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lift_geom_bits.npz")
# mp_lift_fuse_path takes the rotation and the view test from the header, in its tables and emit kernels, which work frame by frame; its scan and
# backtrack kernels take nothing from it.  Of the statement test's 34 scenes every (V, K, C), quaternion and valid-table combination is kept at one
# of its two path settings (alternating), and the 4096-state take.  The 1100-frame take, the only one of several backtrack chunks, is left out for the
# recording's size: chunks exist in the scan alone, which this recording does not guard (test_gpu_lift_fuse_path.py holds it to the statement)
PATH_KEEP = tuple(n for n in range(32) if n % 2 == (n // 2) % 2) + (32,)
SCORE_CASES = ((5, 17, 4, True), (1, 3, 3, False))      # Procrustes-flagged; M = 3 is the fewest joints the entry point aligns


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(prefix, names, res):
    torch.cuda.synchronize()
    return {f"{prefix}_{k}": r.cpu().numpy() for k, r in zip(names, res) if r is not None}


def _nested(quat, trans, intr):
    return [[np.concatenate([intr[g, v], quat[g, v], trans[g, v]]) for v in range(quat.shape[1])] for g in range(quat.shape[0])]


def record_fuse():
    from manipose_amd import fuse_views
    out = {}
    for n, (_, hyps, quat, valid, off, _) in enumerate(lift_fuse_ref.fuse_cases()):
        out.update(_host(f"fuse{n}", ("pose", "choice", "cost", "spread", "ok"), fuse_views(_dev(hyps), quat, _dev(valid), off, 0.02, 1.0)))
    return out


def record_fuse_place():
    from manipose_amd import place_views
    names = ("root", "reproj", "ok", "steps")
    out = {}
    for n, (_, pose, kp, cams, valid, off, weights, distort, iters, _, _) in enumerate(lift_fuse_ref.place_cases()):
        out.update(_host(f"place{n}", names, place_views(_dev(pose), _dev(kp), _nested(*cams), _dev(valid), off, weights, bool(distort), iters, return_steps=True)))
    pose, kp, cams, off, valid = lift_fuse_ref.degenerate_place_scene()
    one = np.zeros((4, 8), np.uint8)
    one[0] = 1
    for tag, mask in (("degenerate", valid), ("degenerate_one_view", one)):
        out.update(_host(f"place_{tag}", names, place_views(_dev(pose), _dev(kp), _nested(*cams), _dev(mask), off, None, True, 3, return_steps=True)))
    return out


def record_fuse_path():
    from manipose_amd import fuse_views_path
    out = {}
    cases = lift_fuse_path_ref.path_cases()
    for n in PATH_KEEP:
        _, hyps, quat, valid, off, ps, sw, _ = cases[n]
        out.update(_host(f"path{n}", ("pose", "choice", "cost", "spread", "ok", "path_cost"),
                         fuse_views_path(_dev(hyps), quat, _dev(valid), off, 0.02, 1.0, ps, sw)))
    return out


def record_align():
    from manipose_amd import align_views
    out = {}
    for n, (_, inp, _) in enumerate(lift_align_ref.cases()):
        res = align_views(_dev(inp["poses"]), _dev(inp.get("valid")), inp["off"], _dev(inp.get("traj")), _dev(inp.get("traj_ok")), inp.get("sigma", 0.05),
                          inp.get("iters", 5))
        out.update(_host(f"align{n}", ("quat", "trans", "rms", "trans_rms", "used", "ok"), res))
    return out


def record_bundle():
    from manipose_amd import bundle_views
    out = {}
    scenes = [c[1] for c in lift_bundle_ref.cases()] + [lift_bundle_ref.inputs(lift_bundle_ref.refused_scene(), iters=8)]
    for n, inp in enumerate(scenes):
        a = dict(dict(valid=None, root_ok=None, fixed=None, weights=None, distort=True, sigma=float("inf"), iters=3), **inp)
        res = bundle_views(_dev(a["pose"]), _dev(a["root"]), _dev(a["kp"]), _nested(a["quat"], a["trans"], a["intr"]), _dev(a["valid"]), a["take_offset"],
                           _dev(a["root_ok"]), a["fixed"], a["weights"], a["distort"], a["sigma"], a["iters"])
        out.update(_host(f"bundle{n}", ("quat", "trans", "root", "reproj", "cost", "steps", "ok", "used"), res[1:]))
    return out


def record_score():
    from manipose_amd import _lib
    lib = _lib.load()
    out = {}
    for inner, M, C, rr in SCORE_CASES:
        pred, gt, off = lift_score_ref.case_inputs((inner, M, C, rr))
        valid = lift_score_ref.valid_pattern(off, inner)
        S, R = len(off) - 1, int(lib.mp_lift_score_row_doubles(M))
        n = int(lib.mp_lift_score_scratch_doubles(S, inner, M))
        rows = torch.full((S, inner, R), -7.0, dtype=torch.float64, device="cuda")
        fe = torch.full((pred.shape[0], inner), -7.0, device="cuda")
        scratch = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
        d_pred, d_gt, d_off, d_valid = _dev(pred), _dev(gt), _dev(off), _dev(valid)
        parents = (ctypes.c_int32 * M)(*lift_score_ref.H36M_PARENTS) if M == 17 else None
        flags = lift_score_ref.PROCRUSTES | (lift_score_ref.ROOT_RELATIVE if rr else 0)
        _lib.check(lib.mp_lift_score(_lib.ptr(d_pred), pred.shape[0], inner, M, C, _lib.ptr(d_gt), _lib.ptr(d_valid), _lib.ptr(d_off), S, parents, 1.0, 1.0,
                                     flags, _lib.ptr(rows), _lib.ptr(fe), _lib.ptr(scratch), n, None), "mp_lift_score")
        out.update(_host(f"score_M{M}", ("rows", "frame_err"), (rows, fe)))
    return out


RECORDERS = (record_fuse, record_fuse_place, record_fuse_path, record_align, record_bundle, record_score)


def _holds(prefix, got):
    """every recorded array of this entry point, byte for byte; returns the recording's own arrays of that entry point"""
    gold = np.load(GOLD)
    want = {k: gold[k] for k in gold.files if k.startswith(prefix)}
    assert sorted(want) == sorted(got)
    for k, a in got.items():
        assert a.dtype == want[k].dtype and a.shape == want[k].shape and a.tobytes() == want[k].tobytes(), k
    return want


def _all(want, field):
    return np.concatenate([v.reshape(-1) for k, v in want.items() if k.endswith("_" + field)])


def test_fuse_has_the_recorded_bits():
    want = _holds("fuse", record_fuse())
    choice, ok = _all(want, "choice"), _all(want, "ok")
    assert (choice == 255).any() and (choice < 8).any() and (ok == 0).any() and (ok == 1).any()       # masked views, and frames no view sees


def test_fuse_place_has_the_recorded_bits():
    want = _holds("place", record_fuse_place())
    ok, steps = _all(want, "ok"), _all(want, "steps")
    assert (ok == 0).any() and (ok == 1).any() and (steps == 0).any() and (steps == 3).any()       # degenerate fits, a joint behind a camera, full steps
    assert want["place_degenerate_ok"][lift_fuse_ref.BEHIND] == 0 and want["place_degenerate_root"][lift_fuse_ref.BEHIND].any()


def test_fuse_path_has_the_recorded_bits():
    want = _holds("path", record_fuse_path())
    choice, ok = _all(want, "choice"), _all(want, "ok")
    assert (choice == 255).any() and (choice < 8).any() and (ok == 0).any() and (ok == 1).any() and np.isfinite(_all(want, "path_cost")).all()


def test_align_views_has_the_recorded_bits():
    want = _holds("align", record_align())
    ok = _all(want, "ok")
    assert (ok == 0).any() and (ok == 1).any() and (ok == 3).any() and (_all(want, "rms") > 0).any()         # missing views, with and without traj


def test_bundle_views_has_the_recorded_bits():
    want = _holds("bundle", record_bundle())
    steps = _all(want, "steps")
    assert (steps == 0).any() and (steps == 3).any() and (steps == 8).any() and _all(want, "ok").all()
    last = len(lift_bundle_ref.cases())
    assert want[f"bundle{last}_steps"].tolist() == [1]                      # the refused scene: the second of eight steps is not taken


def test_score_has_the_recorded_bits():
    want = _holds("score", record_score())
    for M in (17, 3):
        rows, fe = want[f"score_M{M}_rows"], want[f"score_M{M}_frame_err"]
        assert (rows[..., 7] > 0).all() and (fe == -1).any() and (fe > 0).any()          # aligned sums; frames counted and not counted
