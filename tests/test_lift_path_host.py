"""Lifting along one hypothesis path, the host side (no GPU): the numpy statement of the rule (lift_path_ref.py) against the enumeration of all
K^N paths, the conditions the GPU tests' inputs must meet for an exact comparison of paths (margin) and for saying something (coverage), the new
entry points of the C ABI in the places that declare them, the config keys, and every argument error of lift_sequences, select_path and of the
entry point, which are raised before anything touches a device."""
import os
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import lift_path_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


@pytest.mark.parametrize("K,N,J,sigma,switch", [(3, 6, 17, 0.02, 0.0), (2, 9, 2, 0.005, 0.3), (3, 6, 4, 0.1, 1.0), (4, 1, 3, 0.02, 0.0), (2, 9, 17, np.inf, 0.0)])
def test_the_statement_equals_brute_force(K, N, J, sigma, switch):
    for seed in range(4):
        hyps, _ = ref.path_inputs([N], K, J, 100 + seed)
        path, out, cost, margin, covered = ref.select_all(hyps, None, sigma, switch)
        want_path, want_cost = ref.brute_force(ref.unary(hyps), ref.transitions(hyps, sigma, switch))
        assert margin[0] > 0 and covered.all()                               # no tie: the minimum is unique
        assert np.array_equal(path, want_path) and cost[0] == want_cost
        assert np.array_equal(out, hyps[np.arange(N), path][:, :, :3])
        # the forced-through table: its minimum over k is the optimum at every frame, attained on the path
        t = ref.through(ref.unary(hyps), ref.transitions(hyps, sigma, switch))
        assert np.abs(t.min(axis=1) - cost[0]).max() <= 1e-12 * max(1.0, abs(cost[0])) and np.array_equal(t.argmin(axis=1), path)


def test_the_rules_of_the_statement():
    hyps, _ = ref.path_inputs([12], 3, 5, 7)
    # sigma = inf, no switch cost: every frame's first best score, exact ties included
    hyps[4, :, :, 3] = np.float32(0.25)
    hyps[7, 1:, :, 3] = hyps[7, 1, 0, 3]
    hyps[7, 0, :, 3] = np.float32(0.0)
    path = ref.select_all(hyps, None, np.inf, 0.0)[0]
    assert np.array_equal(path, ref.best_score(hyps)) and path[4] == 0 and path[7] == 1
    # identical hypotheses with equal scores: all zeros
    same = np.repeat(hyps[:, :1], 3, axis=1)
    assert not ref.select_all(same, None, 0.02, 0.0)[0].any() and not ref.select_all(same, None, 0.02, 0.7)[0].any()
    # a score that is not > 1e-12 counts as 1e-12; a cost that is not finite as 1e30
    bad = hyps.copy()
    bad[3, 0, :, 3] = np.nan
    bad[5, 1, :, 3] = -1.0
    bad[6, 2, :, 3] = 0.0
    U = ref.unary(bad)
    assert U[3, 0] == U[5, 1] == U[6, 2] == -np.log(1e-12) and np.isfinite(U).all()
    bad[9, 2, 3, 1] = np.nan
    D = ref.transitions(bad, 0.02, 0.0)
    assert (D[9, :, 2] == 1e30).all() and (D[10, 2, :] == 1e30).all() and np.isfinite(D).all() and not D[0].any()
    p = ref.select_all(bad, None, 0.02, 0.0)[0]
    assert p[9] != 2 and p[3] != 0
    # two sequences give what each gives alone; a wild table is its clamped form; an empty range has cost 0 and covers nothing
    both = ref.select_all(hyps, [0, 5, 12], 0.02, 0.1)
    a, b = ref.select_all(hyps[:5], None, 0.02, 0.1), ref.select_all(hyps[5:], None, 0.02, 0.1)
    assert np.array_equal(both[0], np.concatenate([a[0], b[0]])) and both[2].tolist() == [a[2][0], b[2][0]]
    wild = ref.select_all(hyps, [-5, 5, 10 ** 12], 0.02, 0.1)
    assert np.array_equal(wild[0], both[0]) and np.array_equal(wild[2], both[2])
    assert ref.clamp_offsets([3, 3, 2, 40], 12) == [(3, 3), (3, 3), (2, 12)]
    empty = ref.select_all(hyps, [0, 12, 12], 0.02, 0.1)
    assert empty[2][1] == 0.0 and np.array_equal(empty[0], ref.select_all(hyps, None, 0.02, 0.1)[0])
    part = ref.select_all(hyps, [2, 9], 0.02, 0.1)
    assert part[4].tolist() == [False] * 2 + [True] * 7 + [False] * 3


def test_margin_and_coverage_of_the_gpu_tests_inputs():
    """The GPU test compares paths exactly.  That is justified only where no alternative path comes within the rounding of the kernel's fp64
    arithmetic (about N (3 J + 8) 2^-53 relative, 4e-12 at N = 300) of the optimum: every input must keep a margin of 1e-8 max(1, optimum)."""
    print()
    many_switches = constant = False
    for case in ref.GPU_CASES:
        lens, K, J, sigma, switch, _ = case
        hyps, off = ref.case_inputs(case)
        path, out, cost, margin, covered = ref.select_all(hyps, off, sigma, switch)
        ranges = ref.clamp_offsets(off, len(hyps))
        sw = ref.switches(path, ranges)
        differs = path != ref.best_score(hyps)
        rel = [margin[s] / max(1.0, abs(cost[s])) for s in range(len(lens))]
        print(f"[{ref.case_id(case)}] relative margin >= {min(rel):.2e}; switches per sequence {sw}; differs from best_score in "
              f"{[round(float(differs[f0:f1].mean()), 2) for f0, f1 in ranges]} of the frames")
        assert covered.all() and np.isfinite(cost).all()
        if K > 1:
            assert min(rel) >= 1e-8
            assert np.array_equal(path, ref.select_all(hyps, off, sigma, switch, reverse_joints=True)[0])        # the joint sum's order does not matter
            many_switches |= any(n >= 3 and differs[f0:f1].mean() >= 0.25 for n, (f0, f1) in zip(sw, ranges))
            constant |= any(n == 0 and f1 - f0 >= 30 for n, (f0, f1) in zip(sw, ranges))
        else:
            assert not path.any()
    assert many_switches and constant
    assert {c[1] for c in ref.GPU_CASES} >= {1, 2, 3, 5, 8} and {c[2] for c in ref.GPU_CASES} == {2, 17, 32}
    assert any(c[4] == 0 for c in ref.GPU_CASES) and any(c[4] > 0 for c in ref.GPU_CASES)
    assert all(1 in c[0] and len(c[0]) > 1 for c in ref.GPU_CASES) and any(2 in c[0] for c in ref.GPU_CASES)


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = _lib.declared_symbols()
    assert "mp_lift_path" in declared and "mp_lift_path_scratch_floats" in declared
    assert len(_lib._SIGNATURES["mp_lift_path"][1]) == 14 and len(_lib._SIGNATURES["mp_lift_path_scratch_floats"][1]) == 2
    assert _lib._SIGNATURES["mp_lift_path_scratch_floats"][0] is _lib.i64
    assert "lib.mp_lift_path.argtypes" in doc and "lib.mp_lift_path_scratch_floats.argtypes" in doc
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    chunk = int(re.search(r"#define MP_LIFT_PATH_CHUNK (\d+)", header).group(1))
    assert 1 <= chunk <= 1024
    assert lifting.AGG == {"weighted_ave": 0, "best_score": 1}                   # mp_lift_merge's two: the path is not an aggregation of the merge
    assert manipose_amd.select_path is lifting.select_path and "select_path" in lifting.__all__
    assert lifting._Lifted._fields == ("poses", "hyps", "bones", "place", "path", "score", "rotations")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_path.hip"))
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "mp_lift_path") and lib.mp_lift_path_scratch_floats(550000, 5) == 550000 * (8 * 25 + 9 * 5) // 4
        assert lib.mp_lift_path_scratch_floats(3, 1) == (3 * 17 + 3) // 4 and lib.mp_lift_path_scratch_floats(0, 5) == 0


def test_config_keys_parse_a_typo_fails_and_the_readme_command_parses():
    from _entry import LIFT_SUFFIXES, lift_path_options, load_config
    cfg = load_config([])
    assert cfg.lift.agg == "weighted_ave" and cfg.lift.path_sigma == 0.02 and cfg.lift.path_switch == 0.0
    assert lift_path_options(cfg) == ("weighted_ave", 0.02, 0.0)
    assert lift_path_options(load_config(["lift.agg=best_score"]))[0] == "best_score"
    cfg = load_config(["lift.agg=path", "train.tta=false", "lift.path_sigma=0.05", "lift.path_switch=2"])
    assert lift_path_options(cfg) == ("path", 0.05, 2.0)
    for typo in ("lift.path_sigm=0.1", "lift.pathswitch=1"):
        with pytest.raises(SystemExit):
            load_config([typo])
    assert "__path" in LIFT_SUFFIXES and "__path_cost" in LIFT_SUFFIXES
    lines = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("python hpe/") and "lift.agg=path" in l]
    assert len(lines) == 1
    cfg = load_config(shlex.split(lines[0].split("#")[0])[2:])
    assert cfg.run.lift is True and lift_path_options(cfg)[0] == "path"


def test_entry_point_errors_come_before_the_model_is_built():
    from _entry import run
    ok = ["lift.agg=path", "train.tta=false"]
    for argv, word in ((["lift.agg=path"], "train.tta=false"), (["lift.agg=path", "train.tta=true"], "head k of a mirrored"),
                       (ok + ["model.arch=manifold"], "rmcl_manifold"), (ok + ["model.arch=mixste"], "rmcl_manifold"),
                       (ok + ["multi_hyp.n_hyp=1"], "2..8"), (ok + ["multi_hyp.n_hyp=9"], "2..8"),
                       (ok + ["lift.path_sigma=0"], "must be > 0"), (ok + ["lift.path_sigma=-0.1"], "must be > 0"), (ok + ["lift.path_sigma=big"], "is a number"),
                       (ok + ["lift.path_switch=-1"], "finite and >= 0"), (ok + ["lift.path_switch=true"], "is a number"),
                       (["lift.path_sigma=0.05"], "set lift.agg=path"), (["lift.path_switch=1.5"], "set lift.agg=path"),
                       (["lift.agg=oracle"], "weighted_ave, best_score or path"), (["lift.agg=viterbi"], "weighted_ave, best_score or path")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false", "run.lift=true"] + argv)        # (a run that got further would need a device)


def _cpu_model(n_hyp=2):
    from manipose_amd import ManifoldMixSTE, RMCLManifoldMixSTE, h36m_skeleton
    kw = dict(num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1, num_heads_seg=4)
    return RMCLManifoldMixSTE(h36m_skeleton(), n_hyp=n_hyp, **kw) if n_hyp else ManifoldMixSTE(h36m_skeleton(), **kw)


def test_argument_errors_are_value_errors_before_any_device_work():
    """Every call below is given a CPU model or CPU tensors: had the arguments been accepted, the call would have ended in the RuntimeError that
    refuses them ("no CPU fallback"), which is what the valid calls at the end do."""
    from manipose_amd import lift_sequences, select_path
    from manipose_amd.lifting import merge_windows
    model = _cpu_model()
    seqs = [np.zeros((12, 17, 2), np.float32), np.zeros((20, 17, 2), np.float32)]
    path = dict(agg="path", tta=False)
    for kw, word in ((dict(agg="path"), "head k of a mirrored"), (dict(agg="path", tta=True), "pass tta=False"),
                     (dict(keep_padding=True, **path), "keep_padding"),
                     (dict(path_sigma=0.05), "pass agg='path'"), (dict(path_switch=1.0), "pass agg='path'"), (dict(return_path=True), "pass agg='path'"),
                     (dict(agg="best_score", return_path=True, tta=False), "pass agg='path'"),
                     (dict(path_sigma=0.0, **path), "path_sigma must be > 0"), (dict(path_sigma=-1.0, **path), "path_sigma must be > 0"),
                     (dict(path_sigma=float("nan"), **path), "path_sigma must be > 0"), (dict(path_sigma="0.02", **path), "are numbers"),
                     (dict(path_sigma=True, **path), "are numbers"), (dict(path_switch=-0.5, **path), "path_switch must be finite"),
                     (dict(path_switch=float("inf"), **path), "path_switch must be finite"), (dict(path_switch=float("nan"), **path), "path_switch must be finite"),
                     (dict(path_switch=1e39, **path), "path_switch must be finite"),
                     (dict(agg="oracle"), "agg in"), (dict(agg="viterbi", tta=False), "agg in")):
        with pytest.raises(ValueError, match=word):
            lift_sequences(model, seqs, **kw)
    for single in (_cpu_model(0), _cpu_model(1)):                            # a model of one hypothesis has no path to choose
        with pytest.raises(ValueError, match="this model has 1"):
            lift_sequences(single, seqs, **path)
    for kw in (path, dict(path_sigma=float("inf"), path_switch=3, return_path=True, return_hyps=True, **path),
               dict(smooth_poses=2, rigid=True, return_path=True, **path), dict(path_sigma=0.02, path_switch=0.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lift_sequences(model, seqs, **kw)
    with pytest.raises(ValueError, match="agg must be one of"):             # the merge itself keeps its two names
        merge_windows(None, None, [0], [0], [0, 9], T=9, tta=False, mirror=None, agg="path")
    hyps = torch.zeros(6, 3, 17, 4)
    for args, kw, word in (((hyps,), dict(sigma=0), "sigma must be > 0"), ((hyps,), dict(switch_cost=-1), "switch_cost must be finite"),
                           ((hyps,), dict(sigma=None), "are numbers"), ((torch.zeros(6, 3, 17, 3),), {}, "hyps must be"),
                           ((torch.zeros(6, 17, 4),), {}, "hyps must be"), ((hyps.double(),), {}, "hyps must be"),
                           ((hyps[:, :, :, :].transpose(0, 1),), {}, "hyps must be"), ((torch.zeros(6, 9, 17, 4),), {}, "1..8 expected"),
                           ((torch.zeros(6, 0, 17, 4),), {}, "1..8 expected"), ((torch.zeros(6, 3, 33, 4),), {}, "2..32 expected"),
                           ((torch.zeros(6, 3, 1, 4),), {}, "2..32 expected")):
        with pytest.raises(ValueError, match=word):
            select_path(*args, **kw)
    for args in ((hyps,), (hyps.numpy(),)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            select_path(*args)
