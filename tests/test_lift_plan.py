"""Sequence lifting, the host side (no GPU): the window plan of manipose_amd/lifting.py, the new entry points of the C ABI in the three
places that declare it, and the CPU oracle's composition (rmcl_manifold_forward per window + the numpy stitching of lift_ref.py)
against the reference's own lift_action (tests/golden/lift.npz, made by tools/gen_golden_lift.py)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import manipose_ref as orc
from helpers import GOLDEN, fixture_state, load_fixture
from lift_ref import closed_form_tables, cut_windows, oracle_lift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-5, atol=2e-6)          # tests/test_oracle_golden.py: the oracle's model outputs against the reference's


def _lengths(T):
    return [5, T - 1, T, T + 1, 2 * T, 2 * T + 5, 3000 + T // 2, 4321]


@pytest.mark.parametrize("T", [27, 243])
def test_plan_at_stride_T_is_the_reference_generator_table(T):
    from manipose_amd import plan_windows
    lens = _lengths(T)
    seq, start = plan_windows(lens, T, T)
    assert seq.dtype == np.int32 and start.dtype == np.int32
    to_pose, to_frame = orc.window_tables(lens, T, drop_last=False)             # generators.py:87-104
    assert seq.tolist() == to_pose and start.tolist() == to_frame
    cs, cf = closed_form_tables(lens, T, T)
    assert np.array_equal(seq, cs) and np.array_equal(start, cf)


def test_plan_cuts_the_windows_of_the_reference_generator(golden_dir):
    """The sequences of tests/golden/windows.npz: the plan's windows, replicate padded, ARE what PoseSequenceGenerator(drop_last=False) served."""
    from manipose_amd import plan_windows
    z = np.load(golden_dir + "/windows.npz")
    lens = z["lens"].tolist()
    seq, start = plan_windows(lens, 27, 27)
    assert len(seq) == int(z["strided_pad.len"])
    p2 = [z[f"p2.{i}"] for i in range(len(lens))]
    np.testing.assert_array_equal(cut_windows(p2, seq, start, 27), z["strided_pad.X"])


@pytest.mark.parametrize("T", [27, 243])
def test_plan_with_overlapping_windows(T):
    from manipose_amd import plan_windows
    lens = _lengths(T)
    for stride in (1, T // 2 + 1, T - 1):
        seq, start = plan_windows(lens, T, stride)
        cs, cf = closed_form_tables(lens, T, stride)
        assert np.array_equal(seq, cs) and np.array_equal(start, cf)
        for s, n in enumerate(lens):
            st = start[seq == s]
            assert len(st) == 1 + math.ceil(max(0, n - T) / stride)             # the count formula
            assert st[0] == 0 and np.all(np.diff(st) == stride)
            assert st[-1] < n                                                    # the last window starts inside the sequence
            covered = np.zeros(n, bool)
            for a in st:
                covered[a:a + T] = True
            assert covered.all()                                                 # every frame is covered
        assert np.all(np.diff(seq) >= 0)
    for bad in (0, -1, T + 1):
        with pytest.raises(ValueError):
            plan_windows(lens, T, bad)
    with pytest.raises(ValueError):
        plan_windows([0], T, T)


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib
    names = _lib.declared_symbols()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(_lib.HEADER_PATH).read()
    for sym in ("mp_lift_merge", "mp_lift_windows_2d"):
        assert sym in names and sym in _lib._SIGNATURES
        assert f"lib.{sym}.argtypes" in doc
    assert "hpe/eval_utils.py:226-253" in header and "generators.py:93-104,135-154" in header      # the reference lines it replaces
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8
    import manipose_amd
    assert callable(manipose_amd.lift_sequences) and callable(manipose_amd.lift_action)


def test_lifting_has_no_cpu_fallback():
    from manipose_amd import MixSTE, lift_sequences
    model = MixSTE(num_frame=9, embed_dim=32, depth=1, num_heads=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift_sequences(model, [np.zeros((12, 17, 2), np.float32)])


def test_oracle_composition_matches_the_reference_lift_action():
    """rmcl_manifold_forward per window + aggregate + pose_flip + the numpy stitching, against the reference's lift_action with TTA on:
    the padded frames kept, (windows * T, 17, 3) in metres and (windows * T, K, 17, 4) with return_hyps."""
    fx = load_fixture("lift")
    st, cfg = fixture_state(fx), orc.oracle_cfg(fx["cfg"])
    T = fx["cfg"]["T"]
    p2 = [fx[f"p2.{i}"] for i in range(len(fx["lens"]))]
    assert [len(a) for a in p2] == [5, 2 * T, 2 * T + 5]
    with torch.no_grad():
        outs, hyps = oracle_lift(lambda x: orc.rmcl_manifold_forward(x, st, cfg), p2, T, T, tta=True, keep_padding=True, hyps=True)
    got, got_h = np.concatenate(outs), np.concatenate(hyps)
    assert got.shape == fx["lift"].shape == (6 * T, 17, 3) and got_h.shape == fx["lift_hyps"].shape == (6 * T, fx["cfg"]["n_hyp"], 17, 4)
    np.testing.assert_allclose(got, fx["lift"], **TOL)
    np.testing.assert_allclose(got_h, fx["lift_hyps"], **TOL)
