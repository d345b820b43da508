"""Smoothing lifted sequences in time, the host side (no GPU): the numpy statement of the rule (lift_smooth_ref.py) against the classical
Savitzky-Golay taps, exact polynomial reproduction, the degree rules and numpy.linalg.lstsq; the new entry point of the C ABI in the places that
declare it, the config keys, and every argument error of lift_sequences, smooth_poses, smooth_traj and of the entry point, which are raised before
anything touches a device."""
import os
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import lift_smooth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def test_uniform_quadratic_radius_two_is_the_classical_filter():
    x = np.random.default_rng(0).standard_normal((9, 1, 1, 3)).astype(np.float32)
    c, d = ref.tap_coefficients(range(-2, 3), 2, 2, "uniform")
    assert d == 2 and np.abs(c - np.array([-3, 12, 17, 12, -3]) / 35.0).max() <= 1e-15
    out, filled = ref.smooth_all(x, radius=2, degree=2)
    want = sum(k * x[2 + t:7 + t].astype(np.float64) for k, t in zip(np.array([-3, 12, 17, 12, -3]) / 35.0, range(-2, 3)))
    assert filled.all() and np.abs(out[2:7] - want).max() <= 1e-15           # interior frames
    c, d = ref.tap_coefficients(range(-3, 4), 3, 0, "biweight")              # degree 0: the normalised weights
    w = np.array([ref.taper_weight(t, 3, "biweight") for t in range(-3, 4)])
    assert d == 0 and np.allclose(c, w / w.sum(), rtol=0, atol=1e-16) and (w > 0).all() and w[3] == 1.0


@pytest.mark.parametrize("taper", ["uniform", "biweight"])
@pytest.mark.parametrize("R", [1, 2, 8, 64])
def test_polynomials_are_reproduced_wherever_the_full_degree_is_used(R, taper):
    """integer-valued polynomials of degree <= deg in the frame number (float32 values) come back within 1e-9 at every frame whose fit has the
    full degree - bracketed, n > deg - sequence ends and frames inside a gap included"""
    print()
    for deg in (0, 1, 2):
        x = ref.polynomial_inputs(2, 3, 4, deg)
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() < 2 ** 24
        valid = ref.planted_valid(2, R, deg, seed=5)
        out, filled, used = ref.smooth_all(x, valid, ref.OFF, R, deg, taper, return_degree=True)
        full = used == deg
        one_sided = in_hole = 0                                              # among them: windows at a sequence end or behind a gap, frames inside a hole
        for g, i in zip(*np.nonzero(full)):
            s = int(np.searchsorted(ref.OFF, g, side="right")) - 1
            taus = [t for t in range(-R, R + 1) if ref.OFF[s] <= g + t < ref.OFF[s + 1] and valid[g + t, i]]
            one_sided += min(taus) == 0 or max(taus) == 0
            in_hole += not valid[g, i]
        assert one_sided > 0 or deg > R                                      # (R = 1 has 2 taps at a sequence end: degree 1 at most)
        assert in_hole > 0 or (R == 1 and deg == 2)
        miss = np.abs(out - x)[full][..., :3].max()
        print(f"[polynomial R={R} deg={deg} {taper}] {int(full.sum())} of {full.size} frames at full degree, max |out - x| = {miss:.2e} (bound 1e-9)")
        assert full.sum() > 100 and miss <= 1e-9
        assert np.array_equal(out[..., 3], x[..., 3].astype(np.float64))     # the score channel


def test_the_degree_rules():
    g = np.random.default_rng(1)
    x = g.standard_normal((12, 2, 2, 4)).astype(np.float32)
    x64 = x.astype(np.float64)
    valid = np.ones((12, 2), np.uint8)
    valid[:, 1] = 0                                                          # inner index 1: nothing valid anywhere
    valid[0:2, 0] = 0                                                        # inner index 0: a gap at the start,
    valid[9:12, 0] = 0                                                       # one at the end,
    valid[4:7, 0] = 0                                                        # and frames 4..6 missing in the middle
    out, filled, used = ref.smooth_all(x, valid, None, 1, 2, "uniform", return_degree=True)
    assert not filled[:, 1].any() and np.array_equal(out[:, 1], x64[:, 1]) and (used[:, 1] == -1).all()       # n = 0: a copy, filled = 0
    assert filled[:, 0].tolist() == [0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0] and np.array_equal(out[[0, 5, 10, 11], 0], x64[[0, 5, 10, 11], 0])
    assert used[:, 0].tolist() == [-1, 0, 1, 1, 0, -1, 0, 1, 1, 0, -1, -1]
    assert np.array_equal(out[1, 0, :, :3], x64[2, 0, :, :3]) and np.array_equal(out[9, 0, :, :3], x64[8, 0, :, :3])      # gaps at the ends: held
    assert np.array_equal(out[4, 0, :, :3], x64[3, 0, :, :3]) and np.array_equal(out[6, 0, :, :3], x64[7, 0, :, :3])      # n = 1: the one value
    # n = 2 on both sides of the frame: a straight line through them (deg 2 falls back to 1); n = 2 on one side only: their weighted mean
    line = np.zeros((7, 1, 1, 3), np.float32)
    line[:, 0, 0, 0] = [1, 0, 0, 0, 0, 0, 13]
    v = np.array([1, 0, 0, 0, 0, 0, 1], np.uint8)[:, None]
    out, filled, used = ref.smooth_all(line, v, None, 4, 2, "biweight", return_degree=True)
    assert filled[:, 0].tolist() == [1] * 7 and used[2:5, 0].tolist() == [1, 1, 1] and used[[0, 1, 5, 6], 0].tolist() == [0, 0, 0, 0]
    assert np.abs(out[2:5, 0, 0, 0] - np.array([5, 7, 9])).max() <= 1e-12 and out[1, 0, 0, 0] == 1 and out[5, 0, 0, 0] == 13
    v2 = np.array([0, 0, 1, 1, 0, 0, 0], np.uint8)[:, None]
    line[:, 0, 0, 0] = [9, 9, 2, 4, 9, 9, 9]
    out, filled, used = ref.smooth_all(line, v2, None, 4, 2, "uniform", return_degree=True)
    assert used[:, 0].tolist() == [0, 0, 1, 1, 0, 0, 0] and filled.all()
    assert np.abs(out[[0, 1, 4, 5, 6], 0, 0, 0] - 3.0).max() <= 1e-15 and out[2, 0, 0, 0] == 2 and out[3, 0, 0, 0] == 4       # constant outside
    # a window never crosses a sequence boundary: two sequences give what each gives alone
    both, _ = ref.smooth_all(x, valid, [0, 5, 12], 3, 2, "biweight")
    a, _ = ref.smooth_all(x[:5], valid[:5], None, 3, 2, "biweight")
    b, _ = ref.smooth_all(x[5:], valid[5:], None, 3, 2, "biweight")
    assert np.array_equal(both, np.concatenate([a, b]))


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_statement_agrees_with_lstsq_on_the_gpu_tests_inputs(case):
    """The bound: one thousandth of the unit 2^-23 max(1, |x|) the device is held to against the statement, so the statement's own fp64 error is
    no part of that budget (normal equations of condition below 1e6 leave 1e-10 relative in fp64)."""
    inner, M, C, R, deg, taper = case
    x, valid = ref.smooth_inputs(inner, M, C, R, deg, ref.case_seed(case))
    if M == 32:                                                              # (lstsq over 96 channels per frame: the first joints suffice)
        x = x[:, :, :4]
    own, filled = ref.smooth_all(x, valid, ref.OFF, R, deg, taper)
    other = ref.lstsq_all(x, valid, ref.OFF, R, deg, taper)
    w = ref.worst(own, other)
    print(f"\n[statement vs lstsq {case}] worst difference = {w:.2e} x 2^-23 max(1, |x|) (bound 1e-3); {int((filled == 0).sum())} frames not filled")
    assert w <= 1e-3 and (filled == 0).any() and filled.any()


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mp_lift_smooth" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_smooth"][1]) == 14
    assert "lib.mp_lift_smooth.argtypes" in doc
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_SMOOTH_MAXR (\d+)", header).group(1)) == lifting.SMOOTH_MAXR == 64
    assert lifting.TAPER == ref.TAPER
    for name in ("smooth_poses", "smooth_traj"):
        assert getattr(manipose_amd, name) is getattr(lifting, name) and name in lifting.__all__
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_smooth.hip"))
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_smooth")


def test_config_keys_parse_a_typo_fails_and_the_readme_command_parses():
    from _entry import LIFT_SUFFIXES, lift_smooth_options, load_config
    cfg = load_config([])
    assert cfg.lift.smooth_poses == 0 and cfg.lift.smooth_traj == 0 and cfg.lift.smooth_degree == 2 and cfg.lift.smooth_taper == "uniform"
    assert lift_smooth_options(cfg) == (0, 0, 2, "uniform")
    cfg = load_config(["lift.smooth_poses=4", "lift.smooth_traj=6", "lift.smooth_degree=1", "lift.smooth_taper=biweight", "lift.place=true"])
    assert lift_smooth_options(cfg) == (4, 6, 1, "biweight")
    for typo in ("lift.smooth_pose=4", "lift.smoothtraj=6", "lift.smooth_deg=1"):
        with pytest.raises(SystemExit):
            load_config([typo])
    assert all(s in LIFT_SUFFIXES for s in ("__traj_fit", "__filled", "__hyps_traj_fit", "__hyps_filled"))
    lines = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("python hpe/") and "lift.smooth_poses=" in l]
    assert len(lines) == 1
    cfg = load_config(shlex.split(lines[0].split("#")[0])[2:])
    assert cfg.run.lift is True and lift_smooth_options(cfg)[0] > 0


def test_entry_point_errors_come_before_the_model_is_built():
    from _entry import run
    for argv, word in ((["lift.smooth_poses=65"], "0..64"), (["lift.smooth_poses=-1"], "0..64"), (["lift.smooth_traj=2.5", "lift.place=true"], "0..64"),
                       (["lift.smooth_poses=true"], "0..64"), (["lift.smooth_degree=1"], "describe smoothing"),
                       (["lift.smooth_taper=biweight"], "describe smoothing"), (["lift.smooth_poses=3", "lift.smooth_degree=3"], "0, 1 or 2"),
                       (["lift.smooth_poses=3", "lift.smooth_taper=gauss"], "uniform or biweight"), (["lift.smooth_traj=3"], "lift.place=true"),
                       (["lift.frame=wrold", "lift.smooth_poses=65"], "camera or world")):      # (the place options are checked first)
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false", "run.lift=true"] + argv)        # (a run that got further would need a device)


def _cpu_model():
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    return RMCLManifoldMixSTE(h36m_skeleton(), num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1,
                              num_heads_seg=4, n_hyp=2)


def test_argument_errors_are_value_errors_before_any_device_work():
    """Every call below is given a CPU model or CPU tensors: had the arguments been accepted, the call would have ended in the RuntimeError that
    refuses them ("no CPU fallback"), which is what the valid calls at the end do."""
    from manipose_amd import lift_sequences, smooth_poses, smooth_traj
    from manipose_amd.data.ingest import h36m_cameras
    model = _cpu_model()
    seqs = [np.zeros((12, 17, 2), np.float32), np.zeros((20, 17, 2), np.float32)]
    cams = h36m_cameras()["S11"][:2]
    placed = dict(place=True, cameras=cams)
    for kw, word in ((dict(smooth_poses=65), "smooth_poses is a radius"), (dict(smooth_poses=-1), "smooth_poses is a radius"),
                     (dict(smooth_poses=2.0), "smooth_poses is a radius"), (dict(smooth_poses=True), "smooth_poses is a radius"),
                     (dict(smooth_traj=65, **placed), "smooth_traj is a radius"), (dict(smooth_degree=1), "describe smoothing"),
                     (dict(smooth_taper="biweight"), "describe smoothing"), (dict(smooth_poses=3, smooth_degree=3), "degree must be"),
                     (dict(smooth_poses=3, smooth_degree=-1), "degree must be"), (dict(smooth_traj=3, smooth_taper="gauss", **placed), "taper must be"),
                     (dict(smooth_traj=3), "pass place=True"), (dict(smooth_traj=3, cameras=cams, frame="world"), "pass place=True"),
                     (dict(smooth_poses=3, keep_padding=True), "keep_padding"),
                     # the order: radius, degree / taper without a radius, degree, taper, smooth_traj without place, keep_padding; all after place's
                     (dict(smooth_poses=65, smooth_degree=3), "smooth_poses is a radius"), (dict(smooth_degree=3), "describe smoothing"),
                     (dict(smooth_traj=3, smooth_degree=3, smooth_taper="gauss"), "degree must be"), (dict(smooth_traj=3, smooth_taper="gauss"), "taper must be"),
                     (dict(smooth_traj=3, keep_padding=True), "pass place=True"), (dict(smooth_poses=65, place=True), "place=True needs cameras")):
        with pytest.raises(ValueError, match=word):
            lift_sequences(model, seqs, **kw)
    for kw in (dict(smooth_poses=4), dict(smooth_poses=64, smooth_degree=0, smooth_taper="biweight", rigid=True, return_hyps=True),
               dict(smooth_traj=6, smooth_poses=2, return_place=True, frame="world", floor=True, **placed), dict(smooth_poses=0, smooth_traj=0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lift_sequences(model, seqs, **kw)
    poses, traj, ok = torch.zeros(4, 17, 3), torch.zeros(4, 2, 3), torch.ones(4, 2, dtype=torch.uint8)
    for fn, args, kw, word in ((smooth_poses, (poses,), dict(radius=0), "radius must be"), (smooth_poses, (poses,), dict(radius=65), "radius must be"),
                               (smooth_poses, (poses,), dict(degree=3), "degree must be"), (smooth_poses, (poses,), dict(taper="gauss"), "taper must be"),
                               (smooth_poses, (torch.zeros(4, 17, 2),), {}, "poses must be"), (smooth_poses, (poses.double(),), {}, "poses must be"),
                               (smooth_poses, (torch.zeros(4, 2, 33, 3),), {}, "2..32"),
                               (smooth_traj, (traj,), dict(radius=2.5), "radius must be"), (smooth_traj, (traj,), dict(taper=1), "taper must be"),
                               (smooth_traj, (torch.zeros(4, 2, 4),), {}, "traj must be"), (smooth_traj, (torch.zeros(4),), {}, "traj must be"),
                               (smooth_traj, (traj.double(),), {}, "traj must be"), (smooth_traj, (traj, ok[:, 0]), {}, "ok must be"),
                               (smooth_traj, (traj, ok.float()), {}, "ok must be"), (smooth_traj, (traj, np.ones((4, 2), np.uint8)), {}, "ok must be")):
        with pytest.raises(ValueError, match=word):
            fn(*args, **kw)
    for fn, args in ((smooth_poses, (poses,)), (smooth_poses, (poses.numpy(),)), (smooth_traj, (traj, ok)), (smooth_traj, (traj[:, 0].contiguous(),)),
                     (smooth_traj, (traj.numpy(),))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args)
