"""Joint rotations of lifted poses, the host side (no GPU): the float64 statement of mp_lift_rotations' rule (lift_rot_ref.py) closes with the
decoder's forward kinematics, is twist-free, and its continuity rule equals the sequential sign walk; the decision margins of every scene the GPU
tests use; the new entry point in the places that declare it, the config keys, and the argument errors that are raised before anything touches a
device."""
import os
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import lift_rot_ref as ref
from helpers import load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
PAR, REST = ref.H36M_PARENTS, ref.H36M_REST


def test_statement_round_trip_in_fp64():
    """fk(ik(p), measured lengths) == p to 1e-12 m.  Measured when written: 1.4e-15 m on the fixture (poses made by the reference's forward
    kinematics), 4.5e-8 m through float32-rounded rot6d.  The fixture's poses 0 and 1 have a zero-length bone each and its raw `bones` are signed, so lengths
    are measured from the poses."""
    poses, _ = ref.rigid_h36m_poses(64)
    fx = load_fixture("decoder")["poses"].astype(np.float64)
    short = (ref.measured_lengths(fx, PAR) == 0).any(-1)
    assert fx.shape == (21, 17, 3) and short.tolist() == [True, True] + [False] * 19      # (pose 1: the joint the decoder test excludes)
    print()
    for tag, p in (("random rigid H36M poses", poses), ("the decoder fixture's poses", fx)):
        r = ref.ik(p, PAR, REST)
        L = ref.measured_lengths(p, PAR)
        back = ref.fk_quat(r["quat"], L, PAR, REST, p[:, 0])
        back6 = ref.fk_rot6d(r["rot6d"], L, PAR, REST, p[:, 0])
        back32 = ref.fk_rot6d(r["rot6d"].astype(np.float32), L, PAR, REST, p[:, 0])
        e, e6, e32 = np.abs(back - p).max(), np.abs(back6 - p).max(), np.abs(back32 - p).max()
        print(f"[round trip] {tag}: quaternions {e:.2e} m, rot6d {e6:.2e} m (bound 1e-12); float32-rounded rot6d {e32:.2e} m")
        assert e <= 1e-12 and e6 <= 1e-12 and e32 <= 1e-6
        assert np.abs(np.sqrt((r["quat"] ** 2).sum(-1)) - 1).max() <= 1e-15 * 4
    assert ref.ik(poses, PAR, REST)["ok"].all() and np.array_equal(ref.ik(fx, PAR, REST)["ok"] == 0, short)      # ok = 0: the bone without a direction
    for kind in ("pair", "chain"):                                        # no second reference bone: the root is an arc, and the closure holds
        P, off, par, rest = ref.random_scene(kind, 1, 3, seed=2)
        p = P[:, 0].astype(np.float64)
        back = ref.fk_quat(ref.ik(p, par, rest)["quat"], ref.measured_lengths(p, par), par, rest, p[:, 0])
        assert np.abs(back - p).max() <= 1e-12, kind


def test_rotations_are_twist_free():
    poses, _ = ref.rigid_h36m_poses(64, seed=8)
    tb = ref.tables(PAR, REST)
    r = ref.ik(poses, PAR, REST)
    axis_along_bone = np.abs((r["quat"][:, 1:, 1:] * tb["rest"][1:]).sum(-1)).max()
    print(f"\n[twist] |axis . rest| <= {axis_along_bone:.2e} (bound 1e-15)")
    assert axis_along_bone <= 1e-15                                       # q[j]'s axis is perpendicular to rest_j: no rotation about the bone
    R0 = ref.matrix(r["quat"][:, 0])
    d_a = poses[:, tb["a"]] - poses[:, 0]
    d_a /= np.sqrt((d_a * d_a).sum(-1))[:, None]
    assert np.abs(R0 @ tb["rest"][tb["a"]] - d_a).max() <= 1e-15 * 8       # the root frame maps rest_a onto d_a
    spine = poses[:, tb["b"]] - poses[:, 0]
    assert (((R0 @ tb["E"][1]) * spine).sum(-1) > 0).all() and np.abs((R0 @ tb["E"][2] * spine).sum(-1)).max() <= 1e-15      # ... and d_b into its half plane


def test_continuity_equals_the_sequential_sign_walk():
    P, off, par, rest = ref.random_scene("h36m", 5, 3, seed=3)
    c = ref.ik(P, par, rest)["quat"].astype(np.float32)
    signed, flips, least = ref.continuity(c, off)
    walk = c.copy()
    for s in range(len(off) - 1):
        for g in range(int(off[s]) + 1, int(off[s + 1])):                 # frame by frame: flip where the dot with the STORED predecessor is negative
            neg = (walk[g].astype(np.float64) * walk[g - 1].astype(np.float64)).sum(-1) < 0
            walk[g] = np.where(neg[..., None], -walk[g], walk[g])
    assert np.array_equal(signed, walk) and 0.2 < flips.mean() < 0.6 and least >= ref.MARGIN
    for s in range(len(off) - 1):
        a = signed[int(off[s]):int(off[s + 1])].astype(np.float64)
        assert ((a[1:] * a[:-1]).sum(-1) >= 0).all()
    assert not flips[off[:-1]].any()                                      # every sequence starts on the canonical sign
    assert np.array_equal(ref.matrix(signed.astype(np.float64)), ref.matrix(c.astype(np.float64)))       # q and -q are one rotation
    P, off = ref.alternating_scene()
    _, _, _, flips, m = ref.rotations(P, PAR, REST, off)
    assert np.array_equal(flips[:, 0, 0], np.arange(70) % 2 == 1) and not flips[:, 0, 1:].any() and m["dot"] >= 0.9


def test_margins_of_the_gpu_inputs():
    """Every decision the statement takes on the scenes of test_gpu_lift_rot.py lies at least 1e-3 from its threshold; the constructed cases sit
    exactly ON theirs, in numbers that are exact in binary arithmetic."""
    print()
    for kind, inner, ch in ref.SCENES:
        P, off, par, rest = ref.random_scene(kind, inner, ch)
        assert P.shape == (200, inner, len(par), ch) and off.tolist() == [0, 1, 3, 70, 200]
        _, _, ok, flips, m = ref.rotations(P, par, rest, off)
        ref.check_margins(f"{kind} inner={inner} C={ch}", m, need_frame=kind == "h36m")
        assert ok.all() and flips.any() and (np.isfinite(m["frame"]) == (kind == "h36m"))
    P, off = ref.alternating_scene()
    ref.check_margins("alternating hemispheres", ref.rotations(P, PAR, REST, off)[4])
    poses, quat, rot6d, ok = ref.exact_scene()
    p = poses[:, 0].astype(np.float64)
    assert 1.0 + ref.tables(PAR, REST)["rest"][2] @ ((p[ref.HALF_TURN, 2] - p[ref.HALF_TURN, 1]) / 0.5) == 0.0      # exactly opposite
    assert np.array_equal(p[ref.ZERO_BONE, 5], p[ref.ZERO_BONE, 4]) and np.isnan(p[ref.NAN_COORD]).sum() == 1
    d_a, d_b = p[ref.COLLINEAR, 1] / 0.5, p[ref.COLLINEAR, 7] / 0.25
    assert np.array_equal(d_b - (d_b @ d_a) * d_a, np.zeros(3))           # exactly collinear
    assert ok[:, 0].tolist() == [1, 0, 0, 0, 0] and quat[ref.NAN_COORD, 0, :, 0].tolist() == [1.0] * 17


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mp_lift_rotations" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_rotations"][1]) == 14
    assert "lib.mp_lift_rotations.argtypes" in doc
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_ROT_CONTINUOUS (\d+)", header).group(1)) == lifting.ROT_CONTINUOUS == 1
    assert manipose_amd.pose_rotations is lifting.pose_rotations and "pose_rotations" in lifting.__all__
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_rot.hip"))
    assert lifting._Lifted._fields == ("poses", "hyps", "bones", "place", "path", "score", "rotations")
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_rotations")


def test_config_keys_parse_a_typo_fails_and_the_readme_command_parses():
    from _entry import LIFT_SUFFIXES, lift_rotations_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.rotations is False and cfg.lift.rotations_continuous is True and lift_rotations_options(cfg) == (False, True)
    cfg = load_config(["run.lift=true", "lift.rotations=true", "lift.rotations_continuous=false"])
    assert lift_rotations_options(cfg) == (True, False)
    cfg = load_config(["+data=mpi_inf_3dhp", "run.lift=true", "lift.rotations=true"], {"data.dataset": "3dhp"})      # no camera needed
    assert lift_rotations_options(cfg) == (True, True)
    with pytest.raises(SystemExit):
        load_config(["lift.rotatoins=true"])
    for argv, word in ((["run.lift=false", "lift.rotations=true"], "set run.lift=true"), (["run.lift=true", "lift.rotations=1"], "true or false"),
                       (["run.lift=true", "lift.rotations_continuous=false"], "set lift.rotations=true"),
                       (["run.lift=true", "lift.rotations=true", "lift.rotations_continuous=0"], "true or false")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)             # (a run that got further would need a device)
    assert all(s in LIFT_SUFFIXES for s in ("__quat", "__quat_ok", "__hyps_quat", "__hyps_quat_ok"))
    lines = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("python hpe/") and "lift.rotations=true" in l]
    assert len(lines) == 1
    cfg = load_config(shlex.split(lines[0].split("#")[0])[2:])
    assert cfg.run.lift is True and lift_rotations_options(cfg) == (True, True)


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors and a CPU model: had the arguments been accepted, they would have ended in the RuntimeError that refuses them
    ("no CPU fallback"), which is what the valid calls at the end do."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton, lift_sequences, pose_rotations
    poses = torch.zeros(4, 17, 3)
    for bad, word in ((torch.zeros(4, 17, 2), "poses must be"), (torch.zeros(4, 17, 3, dtype=torch.float64), "poses must be"),
                      (torch.zeros(4, 2, 17, 5), "poses must be"), (torch.zeros(4, 1, 3), "2..32"), (torch.zeros(4, 12, 3), "default skeleton")):
        with pytest.raises(ValueError, match=word):
            pose_rotations(bad)
    par, rest = ref.skeleton("chain")
    with pytest.raises(ValueError, match="17 joints, but the skeleton has 32"):
        pose_rotations(poses, skeleton=ref.Sk(par, rest))
    with pytest.raises(ValueError, match="parents must precede"):
        pose_rotations(torch.zeros(4, 3, 3), skeleton=ref.Sk((-1, 2, 0), np.ones((3, 3))))
    for row, word in (((0, 0, 0), "finite and not zero"), ((np.nan, 0, 1), "finite and not zero"), ((np.inf, 0, 1), "finite and not zero"),
                      ((1e300, 0, 0), "finite and not zero")):
        broken = rest.astype(np.float64)
        broken[5] = row
        sk = ref.Sk(par, rest)
        sk.t_pose_operators[5] = broken[5]
        with pytest.raises(ValueError, match=word):
            pose_rotations(torch.zeros(4, 32, 3), skeleton=sk)
    sk = ref.Sk(par, rest)
    del sk.t_pose_operators[7]
    with pytest.raises(ValueError, match="no direction for joint 7"):
        pose_rotations(torch.zeros(4, 32, 3), skeleton=sk)
    for good in (lambda: pose_rotations(poses), lambda: pose_rotations(torch.zeros(4, 2, 32, 4), skeleton=ref.Sk(par, rest), return_rot6d=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            good()
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1, num_heads_seg=4,
                               n_hyp=2)
    seqs = [np.zeros((12, 17, 2), np.float32), np.zeros((20, 17, 2), np.float32)]
    for kw, word in ((dict(return_rotations=True), "pass rotations=True"), (dict(rotations_continuous=False), "pass rotations=True"),
                     (dict(rotations=1), "switches"), (dict(rotations=True, keep_padding=True), "keep_padding")):
        with pytest.raises(ValueError, match=word):
            lift_sequences(model, seqs, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift_sequences(model, seqs, rotations=True, rotations_continuous=False, return_rotations=True, rigid=True, return_bones=True)
