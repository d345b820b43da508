"""Rigid lifting, the host side (no GPU): the numpy statement of the projection (lift_rigid_ref.py), the new config keys, the new entry points of
the C ABI in the places that declare them, and the argument errors of lift_sequences, which are raised before anything touches a device."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_rigid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_projection_is_idempotent_and_has_the_table_lengths():
    g = np.random.default_rng(3)
    p = g.standard_normal((6, 17, 3))
    p[2, 5] = p[2, 4]                                                     # a degenerate bone deeper in a chain (joint 5 on its parent 4)
    p[3, 7] = p[3, 0]                                                     # ... and one off the root
    L = g.uniform(0.05, 0.6, (2, 16))
    off = [0, 4, 6]
    once = ref.project_all(p, L, off)
    twice = ref.project_all(once, L, off)
    np.testing.assert_allclose(twice, once, rtol=0, atol=1e-14)          # fp64 roundings of a chain of five bones of ~0.5 m
    assert np.array_equal(once[:, 0], p[:, 0])                            # the root stays
    bl = ref.bone_lengths(once)
    np.testing.assert_allclose(bl[:4], np.broadcast_to(L[0], (4, 16)), rtol=0, atol=1e-14)
    np.testing.assert_allclose(bl[4:], np.broadcast_to(L[1], (2, 16)), rtol=0, atol=1e-14)
    # the fallback rule: joint 5 continues the bone 0 -> 4, joint 7 goes up the z axis
    u4 = (p[2, 4] - p[2, 0]) / np.linalg.norm(p[2, 4] - p[2, 0])
    np.testing.assert_allclose(once[2, 5] - once[2, 4], L[0, 4] * u4, rtol=0, atol=1e-14)
    np.testing.assert_allclose(once[3, 7] - once[3, 0], [0, 0, L[0, 6]], rtol=0, atol=1e-14)
    # directions of the ordinary bones are kept
    d0, d1 = p[0, 1:] - p[0, list(ref.PARENTS[1:])], once[0, 1:] - once[0, list(ref.PARENTS[1:])]
    cos = (d0 * d1).sum(-1) / np.linalg.norm(d0, axis=-1) / np.linalg.norm(d1, axis=-1)
    np.testing.assert_allclose(cos, 1.0, rtol=0, atol=1e-12)


def test_reference_tables_are_the_skeletons():
    from manipose_amd import h36m_skeleton
    sk = h36m_skeleton()
    assert tuple(int(p) for p in sk.parents) == ref.PARENTS
    assert tuple(sk.bones_left) == ref.BONES_LEFT and tuple(sk.bones_right) == ref.BONES_RIGHT
    assert [b[0] for b in sk.bones] == list(range(1, 17))                 # bone b joins joint b + 1 to its parent


def test_config_keys_load_with_their_defaults_and_accept_overrides():
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import load_config
    cfg = load_config([])
    assert cfg.lift.rigid is False and cfg.lift.lengths is None and cfg.lift.symmetric is False
    cfg = load_config(["lift.rigid=true", "lift.lengths=measured", "lift.symmetric=true"])
    assert cfg.lift.rigid is True and cfg.lift.lengths == "measured" and cfg.lift.symmetric is True
    assert load_config(["lift.lengths=model"]).lift.lengths == "model"
    assert load_config(["+data=mpi_inf_3dhp", "lift.rigid=true"]).lift.rigid is True       # the 3DHP entry point reads the same group


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib
    names = _lib.declared_symbols()
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym, nargs in (("mp_lift_rigid", 10), ("mp_bone_length_means", 9)):
        assert sym in names and sym in _lib._SIGNATURES and len(_lib._SIGNATURES[sym][1]) == nargs
        assert f"lib.{sym}.argtypes" in doc
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    import manipose_amd
    from manipose_amd import lifting
    assert callable(manipose_amd.project_rigid) and manipose_amd.project_rigid is lifting.project_rigid
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_rigid.hip"))
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "mp_lift_rigid") and hasattr(lib, "mp_bone_length_means")


def _cpu_models():
    from manipose_amd import MixSTE, RMCLManifoldMixSTE, h36m_skeleton
    rmcl = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1,
                              num_heads_seg=4, n_hyp=2)
    return rmcl, MixSTE(num_frame=9, embed_dim=32, depth=1, num_heads=4)


def test_argument_errors_are_value_errors_before_any_device_work():
    """Every call below is given a CPU model: had the arguments been accepted, the call would have ended in the RuntimeError that refuses a CPU
    model ("no CPU fallback"), which is what the valid calls at the end do."""
    from manipose_amd import lift_sequences, project_rigid
    rmcl, mixste = _cpu_models()
    seqs = [np.zeros((12, 17, 2), np.float32), np.zeros((20, 17, 2), np.float32)]
    with pytest.raises(ValueError, match="MixSTE predicts no bone lengths"):
        lift_sequences(mixste, seqs, rigid=True, lengths="model")
    with pytest.raises(ValueError, match="lengths must be"):
        lift_sequences(rmcl, seqs, rigid=True, lengths="median")
    for bad in (np.ones(15), np.ones((3, 16)), np.ones((2, 17)), np.ones((2, 16, 1)), torch.ones(1, 16)):
        with pytest.raises(ValueError, match=r"lengths must be \(2, 16\) or \(16,\)"):
            lift_sequences(rmcl, seqs, rigid=True, lengths=bad)
    for bad_value in (-0.1, float("nan"), float("inf")):
        t = np.full((2, 16), 0.3)
        t[1, 7] = bad_value
        with pytest.raises(ValueError, match="finite and non-negative"):
            lift_sequences(rmcl, seqs, rigid=True, lengths=t)
        with pytest.raises(ValueError, match="finite and non-negative"):
            lift_sequences(mixste, seqs, rigid=True, lengths=torch.from_numpy(t[1]))
    for kw in (dict(lengths="measured"), dict(lengths=np.full(16, 0.3)), dict(symmetric=True), dict(return_bones=True)):
        with pytest.raises(ValueError, match="rigid=True"):
            lift_sequences(rmcl, seqs, **kw)
    # valid arguments get as far as the device check
    for model, kw in ((rmcl, dict(rigid=True)), (rmcl, dict(rigid=True, lengths="measured", symmetric=True)), (mixste, dict(rigid=True)),
                      (mixste, dict(rigid=True, lengths=np.full(16, 0.3))), (rmcl, dict(rigid=True, lengths=np.zeros((2, 16)), return_bones=True))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lift_sequences(model, seqs, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        project_rigid(torch.zeros(4, 17, 3), np.full(16, 0.3))
