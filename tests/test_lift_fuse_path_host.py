"""Fusing a take's views along time, the host side (no GPU): the float64 statement of the rule (lift_fuse_path_ref.py) against the enumeration of
all paths; what the feature is for (the mirrored scene: per-frame fusion against the path); the margins of every scene the GPU tests compare; the
new entry points in the places that declare them, the config keys, and the argument errors that are raised before anything touches a device."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_fuse_path_ref as ref
import lift_fuse_ref as fuse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def _tables(V, K, frames, seed, valid=None, path_sigma=0.2, switch_cost=0.3):
    hyps, quat, off = fuse_ref.fuse_scene(V, K, 4, 5, lens=[frames], seed=seed)
    rots = [[fuse_ref.rotation(quat[0][v]) if (valid is None or valid[v][f]) else None for v in range(V)] for f in range(frames)]
    f32 = lambda v: float(np.float32(v))                                          # (the entry point takes its four options as floats)
    return hyps, quat, off, ref.take_tables(hyps, rots, f32(0.02), 1.0, f32(path_sigma), f32(switch_cost))


def test_the_staged_recursion_equals_the_enumeration_of_all_paths():
    """V = 2, K = 2 on 4 frames (4^4 = 256 paths) and V = 3, K = 2 on 3 frames (8^3 = 512), with and without a gap in a view: the staged minimum
    is the minimum over all paths up to the rounding of another order of additions"""
    for V, K, frames, seed in ((2, 2, 4, 1), (3, 2, 3, 2)):
        for valid in (None, np.array([[1] * frames] * (V - 1) + [[1, 0] + [1] * (frames - 2)], np.uint8)):
            hyps, quat, off, (_, E, T, subs) = _tables(V, K, frames, seed, valid)
            path, cost, _ = ref.viterbi(E, T)
            best = ref.exhaustive(E, T)
            assert subs == 0 and abs(cost - best) <= 1e-12 * abs(best), (V, K, cost, best)
            walked = float(E[0][tuple(path[0])])
            for g in range(1, frames):                                            # the emitted path costs what the forward pass says
                walked += sum(float(T[g][v][path[g - 1][v], path[g][v]]) for v in range(V)) + float(E[g][tuple(path[g])])
            assert abs(walked - cost) <= 1e-12 * abs(cost)
            got = ref.path_all(hyps, quat, valid, off, path_sigma=0.2, switch_cost=0.3)
            assert got["path_cost"][0] == cost and np.array_equal(got["choice"][got["choice"] != 255], path[got["choice"] != 255])


def test_the_path_keeps_the_true_body_where_the_frames_on_their_own_flip():
    """mirror_scene(): every frame holds the true pose and its mirrored copy, both consistent in all four cameras; the scores favour the copy in 24
    of the 60 frames.  The statement gives: fuse_all (every frame on its own) right in 36 of 60 frames - wrong in exactly the 24 - and the path
    right in 60 of 60 at path_sigma = 0.02 and switch_cost 0, 0.5 and 2 (margins 17.0, 18.0 and 21.0 to the best other path).  A synthetic scene:
    nothing was measured on real data."""
    sc = ref.mirror_scene()
    frames = sc["truth"].shape[0]
    per_frame = fuse_ref.fuse_all(sc["hyps"], sc["quat"], None, sc["off"])
    wrong = (per_frame["choice"] != sc["truth"]).any(axis=1)
    print(f"[mirror] per frame: right in {int((~wrong).sum())} of {frames} frames; the scores favour the mirrored copy in {int(sc['flipped'].sum())}")
    assert wrong.sum() * 3 >= frames and np.array_equal(wrong, sc["flipped"])
    for sw in (0.0, 0.5, 2.0):
        got = ref.path_all(sc["hyps"], sc["quat"], None, sc["off"], path_sigma=0.02, switch_cost=sw)
        right = (got["choice"] == sc["truth"]).all(axis=1)
        print(f"[mirror] path, switch_cost {sw}: right in {int(right.sum())} of {frames} frames, margin {got['margin'][0]:.2f}")
        assert right.all() and got["ok"].all() and got["margin"][0] >= 1.0
    assert len({tuple(r) for r in sc["truth"].tolist()}) == 4                      # the true indices change three times: the path has to follow


def test_margins_of_the_gpu_inputs():
    """Every comparison scene of test_gpu_lift_fuse_path.py: the best path leads every path that differs from it in a valid digit of some frame by
    at least 1e-8 max(1, |cost|), no table entry was replaced by 1e30 and every frame cost is far below it, so that an ulp of log cannot flip a
    choice or ok."""
    worst = np.inf
    for case in ref.path_cases():
        want = case[-1]
        rel = want["margin"] / np.maximum(1.0, np.abs(want["path_cost"]))
        worst = min(worst, rel.min())
        assert (rel >= 1e-8).all(), case[0]
        assert want["subs"] == 0 and np.abs(want["cost"]).max() < 1e6 and np.abs(want["path_cost"]).max() < 1e9, case[0]
        assert want["written"].all() and want["ok"][(want["choice"] != 255).any(axis=1)].all()
    sc = ref.mirror_scene()
    for sw in (0.0, 0.5, 2.0):
        got = ref.path_all(sc["hyps"], sc["quat"], None, sc["off"], path_sigma=0.02, switch_cost=sw)
        assert got["margin"][0] >= 1e-8 * max(1.0, abs(got["path_cost"][0])) and got["subs"] == 0
    print(f"[margins] mp_lift_fuse_path: margin / max(1, |cost|) at least {worst:.2e} over {len(ref.path_cases())} scenes")
    assert len(ref.path_cases()) == 34
    assert ref.LONG > 2 * ref.CHUNK and (ref.LONG - 2 * ref.CHUNK) % ref.CHUNK != 0      # the long take: more than two backtrack chunks


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = _lib.declared_symbols()
    assert "mp_lift_fuse_path" in declared and "mp_lift_fuse_path_scratch_bytes" in declared
    assert len(_lib._SIGNATURES["mp_lift_fuse_path"][1]) == 23 and len(_lib._SIGNATURES["mp_lift_fuse_path_scratch_bytes"][1]) == 3
    assert "lib.mp_lift_fuse_path.argtypes" in doc and "lib.mp_lift_fuse_path_scratch_bytes.argtypes" in doc
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_FUSE_PATH_CHUNK (\d+)", header).group(1)) == ref.CHUNK
    assert manipose_amd.fuse_views_path is lifting.fuse_views_path and "fuse_views_path" in lifting.__all__
    assert lifting._Lifted._fields == ("poses", "hyps", "bones", "place", "path", "score", "rotations")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_fuse_path.hip"))
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "mp_lift_fuse_path" in text and "not measured on real data" in text.lower()
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "mp_lift_fuse_path")
        for V, F, K in ((1, 7, 1), (2, 1000, 8), (3, 37, 2), (4, 3000, 5), (4, 12, 8)):      # Ftot (8 R + 2 K^V + 2) rounded up to 8
            assert int(lib.mp_lift_fuse_path_scratch_bytes(V, F, K)) == ref.scratch_bytes(V, F, K)
        assert int(lib.mp_lift_fuse_path_scratch_bytes(4, 3000, 5)) == 3000 * (8 * 270 + 2 * 625 + 2)
        assert all(int(lib.mp_lift_fuse_path_scratch_bytes(*a)) == 0 for a in ((0, 6, 5), (5, 6, 5), (4, 0, 5), (4, 6, 0), (4, 6, 9)))


def test_config_keys_parse_and_a_path_without_the_fusion_fails():
    from _entry import LIFT_SUFFIXES, lift_fuse_options, lift_fuse_path_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.fuse_path is False and lift_fuse_path_options(cfg) == (False, 0.02, 0.0) and lift_fuse_options(cfg) == (False, 0.02, 1.0, 3)
    cfg = load_config(["run.lift=true", "lift.fuse=true", "lift.fuse_path=true", "lift.fuse_path_sigma=0.05", "lift.fuse_path_switch=2"])
    assert lift_fuse_path_options(cfg) == (True, 0.05, 2.0)
    with pytest.raises(SystemExit):
        load_config(["lift.fuse_pth=true"])
    on = ["run.lift=true", "lift.fuse=true", "lift.fuse_path=true"]
    for argv, word in ((["run.lift=true", "lift.fuse=true", "lift.fuse_path=1"], "true or false"), (["run.lift=true", "lift.fuse_path=true"], "set lift.fuse=true"),
                       (["lift.fuse_path=true"], "set lift.fuse=true"), (["run.lift=true", "lift.fuse=true", "lift.fuse_path_sigma=0.05"], "set lift.fuse_path=true"),
                       (["run.lift=true", "lift.fuse=true", "lift.fuse_path_switch=1"], "set lift.fuse_path=true"),
                       (on + ["lift.fuse_path_sigma=0"], "> 0"), (on + ["lift.fuse_path_sigma=abc"], "is a number"), (on + ["lift.fuse_path_sigma=true"], "is a number"),
                       (on + ["lift.fuse_path_switch=-1"], ">= 0"), (on + ["lift.fuse_path_switch=inf"], ">= 0")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert "__path_cost" in LIFT_SUFFIXES and "__choice" in LIFT_SUFFIXES


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid call at the end does."""
    from manipose_amd import fuse_views_path
    from manipose_amd.data.ingest import h36m_cameras
    quat = np.stack([c["orientation"] for c in h36m_cameras()["S11"]])
    hyps = torch.zeros(4, 6, 5, 17, 4)
    for bad, word in ((torch.zeros(6, 5, 17, 4), "hyps must be"), (hyps.double(), "hyps must be"), (torch.zeros(5, 6, 5, 17, 4), "views"),
                      (torch.zeros(4, 6, 9, 17, 4), "hypotheses"), (torch.zeros(4, 6, 5, 1, 4), "joints"), (torch.zeros(4, 6, 5, 17, 2), "hyps must be")):
        with pytest.raises(ValueError, match=word):
            fuse_views_path(bad, quat)
    zero = quat.copy()
    zero[2] = 0
    for kw, word in ((dict(orientation=zero), "zero quaternion"), (dict(orientation=quat[:3]), "orientation must be"),
                     (dict(valid=torch.ones(4, 5, dtype=torch.uint8)), "valid must be"), (dict(sigma=0), "sigma must be > 0"),
                     (dict(score_weight=-1), "score_weight must be finite and >= 0"), (dict(path_sigma=0), "path_sigma must be > 0"),
                     (dict(path_sigma=float("nan")), "path_sigma must be > 0"), (dict(path_sigma="a"), "numbers"), (dict(path_sigma=True), "numbers"),
                     (dict(switch_cost=-1), "switch_cost must be finite and >= 0"), (dict(switch_cost=float("inf")), "switch_cost must be finite and >= 0"),
                     (dict(switch_cost=float("nan")), "switch_cost must be finite and >= 0")):
        with pytest.raises(ValueError, match=word):
            fuse_views_path(hyps, **{"orientation": quat, **kw})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fuse_views_path(hyps, np.stack([quat, quat]), torch.ones(4, 6, dtype=torch.uint8), [0, 2, 6], sigma=float("inf"), score_weight=0,
                        path_sigma=float("inf"), switch_cost=3)
