"""mp_lift_euler and the BVH writer without a device: the properties of the float64 statement of the rule (lift_euler_ref.py), every condition
the device bounds of test_gpu_lift_euler.py stand on, the bone-centred hierarchy and the written file read back by an independent reader, the host
side of the binding (argument errors), the config keys of lift.bvh and the new symbol's declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_euler_ref as ref
import lift_retime_ref as rt
import lift_rot_ref as rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
H = 0.5


def _gimbal_matrices(order):
    """exact gimbal poses of an order: R_i(a) R_j(+-90 degrees) R_k(c)"""
    i, j, k = ref.AXES[order]
    g = np.random.default_rng(3)
    return [ref.axis_matrix(i, a) @ ref.axis_matrix(j, sgn * np.pi / 2) @ ref.axis_matrix(k, c) for sgn in (1.0, -1.0) for a, c in g.uniform(-3, 3, (6, 2))]


@pytest.mark.parametrize("order", ref.ORDERS)
def test_angles_recompose_to_the_rotation_and_so_does_the_other_solution(order):
    g = np.random.default_rng(ref.ORDERS.index(order))
    worst, gimbals = 0.0, 0
    mats = list(rot.matrix(rot._random_rotations(g, (300,), np.pi))) + _gimbal_matrices(order)
    mats += [rot.matrix(np.array(q, np.float64)) for q in ((H, H, H, H), (H, -H, H, H), (H, H, -H, H), (H, H, H, -H), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1))]
    for R in mats:
        (al, be, ga), gimbal = ref.angles_of(R, order)
        deg = np.rad2deg([al, be, ga])
        gimbals += gimbal
        assert not gimbal or (ga == 0.0 and abs(abs(deg[1]) - 90) < 1e-4)
        worst = max(worst, np.abs(ref.compose(order, deg) - R).max(), np.abs(ref.compose(order, ref.other(deg)) - R).max())
        assert abs(deg[1]) <= 90 and abs(deg[0]) <= 180 and abs(deg[2]) <= 180          # the canonical solution
    print(f"\n[{order}] |R_i R_j R_k - R| <= {worst:.2e} over {len(mats)} rotations, {gimbals} in the gimbal case; T(c) gives the same rotation")
    assert worst < 1e-12 and gimbals >= 12


def _scan_form(c32, ok, off):
    """the continuity as the header states it for the kernel: per track the votes of every frame against its predecessor, the flips their prefix
    parity, the turns a prefix sum of integers (numpy cumsum over the frames that have a result)"""
    c = np.asarray(c32, np.float32)
    out = c.copy()
    ntot, inner, J = c.shape[:3]
    T = lambda x: np.stack([x[:, 0] + 180.0, 180.0 - x[:, 1], x[:, 2] + 180.0], -1)
    w = lambda x: x - 360.0 * np.floor((x + 180.0) / 360.0)
    d = lambda x, y: (np.abs(w(x[:, 0] - y[:, 0])) + np.abs(w(x[:, 1] - y[:, 1]))) + np.abs(w(x[:, 2] - y[:, 2]))
    for s in range(len(off) - 1):
        f0, f1 = ref.frames_of(off, s, ntot)
        for i in range(inner):
            live = f0 + np.flatnonzero(ok[f0:f1, i] != 0)
            if live.size == 0:
                continue
            for j in range(J):
                x = c[live, i, j].astype(np.float64)
                votes = np.concatenate([[False], d(x[1:], T(x[:-1])) < d(x[1:], x[:-1])])
                flip = (np.cumsum(votes) % 2).astype(bool)
                e = np.where(flip[:, None], T(x), x)
                W = np.concatenate([np.zeros((1, 3)), np.cumsum(-np.rint((e[1:] - e[:-1]) / 360.0), axis=0)])
                out[live, i, j] = (e + 360.0 * W).astype(np.float32) + np.float32(0.0)
    return out


def test_the_walk_is_the_prefix_parity_and_prefix_sum_and_the_greedy_choice():
    sc = ref.take("h36m", 5, seed=8)
    r = ref.solve(sc["quat"], None, sc["valid"], sc["off"], None, None, 1.0, "ZXY", ref.CONTINUOUS)
    assert np.array_equal(_scan_form(r["canonical"], r["ok"], sc["off"]).view(np.uint32), r["stored"].view(np.uint32))
    assert r["margins"]["branch"] > 1e-3                                  # no tie: the greedy walk decides the same
    assert np.abs(ref.greedy(r["canonical"], r["ok"], sc["off"]) - r["stored"].astype(np.float64)).max() <= np.spacing(np.float32(np.abs(r["stored"]).max())) / 2
    moved = np.abs(r["stored"] - r["canonical"]) > 90
    assert moved.any() and not moved[r["ok"] == 0].any()
    # d is unchanged when T is applied to both arguments, which is what makes the pairwise vote the greedy choice
    g = np.random.default_rng(0)
    for x, y in g.uniform(-180, 180, (200, 2, 3)).astype(np.float32).astype(np.float64):
        assert abs(ref.dist(ref.other(x), ref.other(y)) - ref.dist(x, y)) < 1e-9 and abs(ref.dist(ref.other(x), y) - ref.dist(x, ref.other(y))) < 1e-9
    # a sequence's curve starts at its own canonical angles, whatever came before it
    f0 = 0
    for n in sc["lens"]:
        first = f0 + int(np.argmax(r["ok"][f0:f0 + n, 0] != 0))
        assert np.array_equal(r["stored"][first, 0], r["canonical"][first, 0])
        f0 += n


@pytest.mark.parametrize("order", ref.ORDERS)
def test_three_full_turns_about_one_axis_give_a_monotone_curve(order):
    n = 217
    for axis in range(3):
        ang = np.linspace(0.0, 6 * np.pi, n)                               # 5 degrees a frame
        q = np.zeros((n, 1, 2, 4), np.float32)
        q[..., 0] = 1
        q[:, 0, 1, 0], q[:, 0, 1, 1 + axis] = np.cos(ang / 2), np.sin(ang / 2)
        r = ref.solve(q, None, None, [0, n], None, None, 1.0, order, ref.CONTINUOUS)
        ch = ref.AXES[order].index(axis)
        curve = r["stored"][:, 0, 1].astype(np.float64)
        assert (np.diff(curve[:, ch]) > 4.9).all() and abs(curve[-1, ch] - 1080.0) < 1e-3, (order, axis)
        rest = np.delete(curve, ch, axis=1)
        assert np.abs(rest - rest[0]).max() < 1e-3 and (np.abs(r["canonical"]) <= 180).all()


@pytest.mark.parametrize("order", ref.ORDERS)
def test_a_track_through_the_middle_angle_of_90_degrees_has_no_jump(order):
    """An arm raised overhead: be goes 60.5 -> 120.5 degrees of arc, half a degree past 90 at the nearest frame (which no canonical be can follow past 90) while al and ga drift.  The canonical
    curves jump by about 180 degrees where be turns round; the continuous ones move by no more than the motion does."""
    i, j, k = ref.AXES[order]
    n = 61
    t = np.linspace(0.0, 1.0, n)
    al, be, ga = np.deg2rad(20 + 10 * t), np.deg2rad(60.5 + 60 * t), np.deg2rad(-30 + 15 * t)
    M = np.stack([ref.axis_matrix(i, a) @ ref.axis_matrix(j, b) @ ref.axis_matrix(k, c) for a, b, c in zip(al, be, ga)])
    q = np.zeros((n, 1, 2, 4), np.float32)
    q[..., 0] = 1
    q[:, 0, 1] = rot.quat_of(M)
    valid = np.ones((n, 1), np.uint8)
    valid[[29, 30, 31]] = 0                                               # the frames around be = 90 are missing: the predecessor is four frames back
    for v in (None, valid):
        r = ref.solve(q, None, v, [0, n], None, None, 1.0, order, ref.CONTINUOUS)
        live = r["ok"][:, 0] != 0
        canon, curve = r["canonical"][live, 0, 1].astype(np.float64), r["stored"][live, 0, 1].astype(np.float64)
        assert np.abs(np.diff(canon, axis=0)).max() > 150
        gap = 1 if v is None else 4
        assert np.abs(np.diff(curve, axis=0)).max() <= gap * 1.0 + 1e-3   # be moves one degree a frame, al and ga less
        want = np.rad2deg(np.stack([al, be, ga], -1))[live]
        # the curve IS the motion's own (al, be, ga), be beyond 90 included - to the float32 rounding of the quaternions (1.2e-7 radians of
        # rotation) amplified by 1 / cos(be) <= 115 half a degree from the pole: 8e-4 degrees
        assert np.abs(curve - want).max() < 2e-3


def test_every_condition_the_device_bounds_stand_on():
    kinds, inners, orders, flags = set(), set(), set(), set()
    worst = dict(c2=np.inf, cut=np.inf, branch=np.inf, turn=np.inf)
    for cid, kind, inner, order, with_basis, with_root, with_valid, scale in ref.cases():
        sc, basis, shift = ref.scene_of(cid)
        want = ref.solved(cid)
        m = want["margins"]
        worst = {k: min(worst[k], float(m[k])) for k in worst}
        # the gimbal test, the branch cut of al and ga, the branch comparison and the turn rounding: far from their thresholds
        assert m["c2"] >= 1e-6 and m["cut"] >= 1e-6 and m["branch"] >= 1e-3 and m["turn"] >= 1e-6, (cid, m)
        assert sc["lens"] == ref.LENS and (want["ok"] != 3).all()
        assert (want["ok"] == 0).any() == with_valid and ((want["pos"] is None) == (not with_root))
        assert float(np.abs(want["stored"]).max()) > 540 and (np.abs(want["canonical"]) <= 180).all()         # turns pile up
        kinds.add(kind); inners.add(inner); orders.add(order); flags.add((with_basis, with_root, with_valid, scale))
    print(f"\n[margins over the cases] c2 >= {worst['c2']:.2e}, a canonical angle >= {worst['cut']:.2e} degrees from its cut, |d(c, T(c')) - d(c, c')| >= "
          f"{worst['branch']:.3f} degrees, a turn count >= {worst['turn']:.3f} from a tie")
    assert kinds == {"h36m", "pair", "chain"} and inners == {1, 5} and orders == set(ref.ORDERS)
    assert {f[0] for f in flags} == {f[1] for f in flags} == {f[2] for f in flags} == {True, False} and {f[3] for f in flags} == {1.0, 100.0}
    q, valid, off = ref.exact_scene()                                     # the constructed frames: exact in binary
    good = ref.usable(q.astype(np.float64))[0]
    u = q.astype(np.float64)[good]
    M = rot.matrix(u / np.sqrt((u * u).sum(-1))[:, None])
    assert np.isin(M, (-1.0, 0.0, 1.0)).all() and not good.all()


def test_the_device_bound_is_derived_not_measured():
    """One float32 ulp of max(|angle|, 1) degrees.  Both sides evaluate the same few fp64 operations; what may differ is the last bit of a library
    function or of an entry of R, about 2^-52 relative.  An error dR in the entries moves atan2(y, x) by at most |dR| sqrt(2) / sqrt(x^2 + y^2) -
    1 / sqrt(c2) for al, the same with R[i][j]^2 + R[i][i]^2 = c2 for ga - and asin by the same factor.  Allowance: 64 x 2^-52 x 1 / sqrt(c2) radians;
    with c2 >= 1e-6 (asserted over the cases) that is 8.1e-10 degrees, a 147th of one ulp of 1 (1.19e-7): the device's value and the statement's
    round to float32 values at most one ulp apart.  The amplification is measured here beside the allowance."""
    g = np.random.default_rng(4)
    worst_ratio, worst_amp = 0.0, 0.0
    for cid, kind, inner, order, *_ in ref.cases()[:6]:
        sc, basis, shift = ref.scene_of(cid)
        q = sc["quat"][::7, 0].astype(np.float64).reshape(-1, 4)
        M = rot.matrix(q / np.sqrt((q * q).sum(-1))[:, None])
        i, j, k = ref.AXES[order]
        for R in M:
            c2 = R[j][k] ** 2 + R[k][k] ** 2
            dR = 1e-9 * g.uniform(-1, 1, (3, 3))
            a0, a1 = np.array(ref.angles_of(R, order)[0]), np.array(ref.angles_of(R + dR, order)[0])
            amp = float(np.abs(ref.wrap(np.rad2deg(a1 - a0))).max()) / np.rad2deg(1e-9)
            worst_amp, worst_ratio = max(worst_amp, amp), max(worst_ratio, amp * np.sqrt(c2))
    allowance = 64 * 2.0 ** -52 / np.sqrt(1e-6) * ref.DEG
    print(f"\n[amplification] d(angle) / |dR| <= {worst_ratio:.2f} / sqrt(c2) measured (allowed: 2), at most {worst_amp:.1f} on these scenes (allowed: 1000 at "
          f"c2 = 1e-6); allowance {allowance:.2e} degrees = 1 / {2.0 ** -23 / allowance:.0f} of one float32 ulp of 1")
    assert worst_ratio <= 2.0 and allowance < 2.0 ** -23 / 100


def test_hierarchy_is_bone_centred():
    from manipose_amd.bvh import bvh_hierarchy
    sk = ref.named_h36m()
    L = np.random.default_rng(1).uniform(0.1, 0.5, 16)
    nodes = bvh_hierarchy(sk, L, 100.0)
    rest = rot.H36M_REST.astype(np.float64)
    par = rot.H36M_PARENTS
    assert len(nodes) == 17 and len({n["name"] for n in nodes}) == 17 and all(re.fullmatch(r"\S+", n["name"]) for n in nodes)
    at_pelvis = [n for n in nodes[1:] if n["joint"] == 0]
    assert len(at_pelvis) == 3 and all(n["offset"] == [0.0, 0.0, 0.0] and n["parent"] == 0 for n in at_pelvis) and nodes[0]["parent"] == -1
    assert [n["name"] for n in at_pelvis] == ["Hip_RHip", "Hip_LHip", "Hip_Spine"] and nodes[0]["name"] == "Hip" and nodes[2]["name"] == "RHip"
    assert [n["name"] for n in nodes if n["joint"] == 8] == ["Thorax_Neck/Nose", "Thorax_LShoulder", "Thorax_RShoulder"]
    for j in range(1, 17):
        n = nodes[j]
        assert n["parent"] == par[j] and n["joint"] == par[j]
        want = np.zeros(3) if par[j] == 0 else 100.0 * L[par[j] - 1] * rest[par[j]]
        assert np.abs(np.array(n["offset"]) - want).max() < 1e-12         # the offset is the PARENT bone: len_parent rest_parent
        leaf = j not in par
        assert (n["end"] is not None) == leaf and (not leaf or np.abs(np.array(n["end"]) - 100.0 * L[j - 1] * rest[j]).max() < 1e-12)
    bare = rot.Sk(*rot.skeleton("pair"))                                   # a skeleton without names: J<k>
    assert [n["name"] for n in bvh_hierarchy(bare, [0.5])] == ["J0", "J0_J1"]
    sk.joints_names = ["a b"] * 17
    with pytest.raises(ValueError, match="not unique"):
        bvh_hierarchy(sk, L)
    sk.joints_names = [f"joint {k}\tx" for k in range(17)]
    assert bvh_hierarchy(sk, L)[2]["name"] == "joint_1_x"
    for bad, word in ((dict(bones=L[:5]), "bones must be"), (dict(bones=-L), "bones must be"), (dict(scale=0), "scale"), (dict(scale=float("nan")), "scale")):
        with pytest.raises(ValueError, match=word):
            bvh_hierarchy(**dict(dict(skeleton=ref.named_h36m(), bones=L, scale=1.0), **bad))


@pytest.mark.parametrize("order,continuous,with_basis,scale", [("ZXY", True, True, 100.0), ("XYZ", False, False, 1.0), ("YZX", True, True, 1.0), ("ZYX", True, False, 100.0)])
def test_written_file_reads_back_to_the_forward_kinematics(tmp_path, order, continuous, with_basis, scale):
    """The statement's float32 angles through write_bvh and the independent reader against lift_retime_ref's forward kinematics of the same (root,
    quat, bones), moved by basis, shift and scale.  Bound: 4 x the float32 rounding error of those positions, floor 1e-7 m x scale (mp_lift_fk's).
    Measured when written: 0.449, 0.472, 0.542 and 0.388 of the bound."""
    from manipose_amd.bvh import write_bvh
    sc, sk = ref.closure_take(), ref.named_h36m()
    basis, shift = ref.transform(1, 4) if with_basis else (None, None)
    r = ref.solve(sc["quat"], sc["root"], sc["valid"], sc["off"], basis, shift, scale, order, ref.CONTINUOUS if continuous else 0)
    path = os.path.join(str(tmp_path), "take.bvh")
    assert write_bvh(path, sk, sc["bones"], r["stored"][:, 0], r["pos"][:, 0].astype(np.float32), r["ok"][:, 0], 50, order, scale) is True
    f = ref.read_bvh(path)
    got = ref.bvh_joints(f, rot.H36M_PARENTS)
    want, ok = rt.fk(sc["quat"], sc["bones"][None], rot.H36M_PARENTS, rot.H36M_REST, sc["root"], [0, 130])
    want = ref.moved(want[:, 0], None if basis is None else basis[0], None if shift is None else shift[0], scale)
    live = r["ok"][:, 0] != 0
    err, bound = float(np.abs(got[live] - want[live]).max()), ref.closure_bound(want[live], scale)
    print(f"\n[closure {order} continuous={continuous} basis={with_basis} scale={scale:g}] |file - fk| = {err:.3e}, bound {bound:.3e} ({err / bound:.3f})")
    assert ok.all() and 100 < live.sum() < 130 and err <= bound
    assert f["frames"] == 130 and abs(f["frame_time"] - 0.02) < 1e-12 and len(f["nodes"]) == 17
    assert f["nodes"][0]["channels"] == ["Xposition", "Yposition", "Zposition"] + [f"{c}rotation" for c in order]
    assert all(n["channels"] == [f"{c}rotation" for c in order] for n in f["nodes"][1:])
    assert np.array_equal(got, got[ref.row_sources(live)])
    # every number reads back to the float32 it was written from
    cols = [0] + [k for k in range(1, 17)]                               # (H36M's joint order is depth first already)
    rows = np.concatenate([r["pos"][:, 0].astype(np.float32), r["stored"][:, 0][:, cols].reshape(130, -1)], axis=1)[ref.row_sources(live)]
    assert np.array_equal(f["motion"].astype(np.float32).view(np.uint32), rows.view(np.uint32))


def test_invalid_frames_repeat_and_an_empty_take_writes_nothing(tmp_path):
    from manipose_amd.bvh import write_bvh
    sk = ref.named_h36m()
    L = np.full(16, 0.25)
    g = np.random.default_rng(2)
    A, P = g.uniform(-180, 180, (8, 17, 3)).astype(np.float32), g.uniform(-1, 1, (8, 3)).astype(np.float32)
    ok = np.array([0, 0, 1, 3, 0, 1, 0, 0], np.uint8)
    path = os.path.join(str(tmp_path), "a.bvh")
    assert write_bvh(path, sk, L, A, P, ok, 30, "ZXY", 1.0)
    m = ref.read_bvh(path)["motion"].astype(np.float32)
    src = [2, 2, 2, 3, 3, 5, 5, 5]                                        # leading invalid frames repeat the first valid one, later ones the last valid before
    assert np.array_equal(m[:, :3], P[src]) and np.array_equal(m[:, 3:], A[src].reshape(8, -1)) and ref.row_sources(ok != 0).tolist() == src
    assert write_bvh(path, sk, L, torch.from_numpy(A), None, None, 30, "ZXY", 1.0) and not ref.read_bvh(path)["motion"][:, :3].any()
    none = os.path.join(str(tmp_path), "none.bvh")
    assert write_bvh(none, sk, L, A, P, np.zeros(8, np.uint8), 30, "ZXY", 1.0) is False and not os.path.exists(none)
    for bad, word in ((dict(order="ZXZ"), "order"), (dict(fps=0), "fps"), (dict(angles=A[:, :5]), "angles must be"), (dict(pos=P[:3]), "pos must be"),
                      (dict(ok=ok[:3]), "ok must be")):
        with pytest.raises(ValueError, match=word):
            write_bvh(**dict(dict(path=none, skeleton=sk, bones=L, angles=A, pos=P, ok=ok, fps=30, order="ZXY", scale=1.0), **bad))
    assert not os.path.exists(none)


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import euler_from_rotations
    z = torch.zeros
    q, r, v = z(12, 17, 4), z(12, 3), torch.ones(12, dtype=torch.uint8)
    for kw, word in ((dict(quat=z(12, 17)), "quat must be"), (dict(quat=q.double()), "quat must be"), (dict(quat=np.zeros((12, 17, 4))), "quat must be"),
                     (dict(quat=z(12, 1, 4)), "joints"), (dict(quat=z(12, 33, 4)), "joints"), (dict(quat=z(0, 17, 4)), "no frame"), (dict(root=z(12, 4)), "root must be"),
                     (dict(root=r.double()), "root must be"), (dict(valid=v[:5]), "valid must be"), (dict(valid=v.bool()), "valid must be"),
                     (dict(seq_offset=[0]), "seq_offset"), (dict(seq_offset=list(range(14))), "seq_offset"), (dict(order="zxy"), "order must be"),
                     (dict(order="XYX"), "order must be"), (dict(order=4), "order must be"), (dict(scale=0), "scale"), (dict(scale=-1.0), "scale"),
                     (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"), (dict(scale="1"), "scale"), (dict(scale=True), "scale"),
                     (dict(basis=np.zeros(3)), "basis must be"), (dict(basis=np.array([1.0, 0, 0, np.nan])), "basis must be finite"),
                     (dict(shift=np.zeros((2, 3))), "shift must be"), (dict(seq_offset=[0, 5, 12], basis=np.zeros((3, 4))), "basis must be")):
        with pytest.raises(ValueError, match=word):
            euler_from_rotations(**dict(dict(quat=q, root=r, valid=v), **kw))
    for kw in (dict(), dict(order="XYZ", continuous=False, scale=100), dict(quat=z(12, 5, 2, 4), root=None, valid=None, seq_offset=[0, 5, 12], basis=np.ones((2, 4)), shift=np.zeros((2, 3))),
               dict(seq_offset=torch.tensor([0, 12]), basis=[1, 0, 0, 0]), dict(shift=[0, 0, 1.0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            euler_from_rotations(**dict(dict(quat=q, root=r, valid=v), **kw))


def test_config_keys_parse_and_the_refusals_fire():
    from _entry import BVH_DEFAULTS, LIFT_SUFFIXES, bvh_file_name, bvh_turn_up, lift_bvh_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.bvh is False and lift_bvh_options(cfg) == (False, BVH_DEFAULTS)
    assert BVH_DEFAULTS == dict(order="ZXY", up="y", scale=100, continuous=True, fps=0)
    base = ["run.lift=true", "lift.rigid=true", "lift.rotations=true"]
    assert lift_bvh_options(load_config(base + ["lift.bvh=true"])) == (True, dict(order="ZXY", up="y", scale=100.0, continuous=True, fps=50, retimed=False))
    on, kw = lift_bvh_options(load_config(base + ["lift.bvh=true", "lift.retime_fps=30", "lift.bvh_order=XYZ", "lift.bvh_up=z", "lift.bvh_scale=1", "lift.bvh_continuous=false"]))
    assert on and kw == dict(order="XYZ", up="z", scale=1.0, continuous=False, fps=30, retimed=True)
    assert lift_bvh_options(load_config(base + ["lift.bvh=true", "lift.retime_fps=30", "lift.bvh_fps=24"]))[1]["fps"] == 24
    assert lift_bvh_options(load_config(base + ["lift.bvh=true", "data.dataset=3dhp", "lift.bvh_fps=25"]))[1]["fps"] == 25
    with pytest.raises(SystemExit):
        load_config(["lift.bvh_axis=y"])
    on_ = base + ["lift.bvh=true"]
    for argv, word in ((["lift.bvh=true", "lift.rigid=true", "lift.rotations=true"], "set run.lift=true"), (["run.lift=true", "lift.rigid=true", "lift.bvh=true"], "set lift.rotations=true"),
                       (["run.lift=true", "lift.rotations=true", "lift.bvh=true"], "set lift.rigid=true"), (base + ["lift.bvh_order=XYZ"], "set lift.bvh=true"),
                       (base + ["lift.bvh_up=z"], "set lift.bvh=true"), (base + ["lift.bvh_scale=1"], "set lift.bvh=true"), (base + ["lift.bvh_continuous=false"], "set lift.bvh=true"),
                       (base + ["lift.bvh_fps=30"], "set lift.bvh=true"), (base + ["lift.bvh=1"], "true or false"), (on_ + ["lift.bvh_order=ZXZ"], "lift.bvh_order"),
                       (on_ + ["lift.bvh_up=x"], "y or z"), (on_ + ["lift.bvh_scale=0"], "finite number > 0"), (on_ + ["lift.bvh_scale=-2"], "finite number > 0"),
                       (on_ + ["lift.bvh_continuous=2"], "true or false"), (on_ + ["lift.bvh_fps=-1"], "positive integer"), (on_ + ["lift.bvh_fps=29.97"], "positive integer"),
                       (on_ + ["data.dataset=3dhp"], "set lift.bvh_fps")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all(s in LIFT_SUFFIXES for s in ("__bvh_euler", "__bvh_pos", "__bvh_ok"))
    assert bvh_file_name("S9/Walking 1.fused0") == "S9_Walking_1.fused0.bvh"
    # the up-axis turn composed in front: (x, y, z) -> (x, z, -y), in float64
    g = np.random.default_rng(5)
    b = rot._random_rotations(g, (1,), np.pi)[0]
    t, p = g.uniform(-1, 1, 3), g.uniform(-1, 1, 3)
    tb, ts = bvh_turn_up(torch.from_numpy(b), torch.from_numpy(t))
    assert tb.dtype == torch.float64 and ts.dtype == torch.float64
    x = rot.matrix(b) @ p + t
    assert np.abs(rot.matrix(tb.numpy()) @ p + ts.numpy() - np.array([x[0], x[2], -x[1]])).max() < 1e-15 and abs(float(tb.norm()) - 1) < 1e-15


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, bvh, lifting, lift_ops
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mp_lift_euler" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_euler"][1]) == 17
    assert "lib.mp_lift_euler.argtypes = [vp, vp, vp, i64, i32, i32, vp, i32, vp, vp, f32, i32, i32, vp, vp, vp, vp]" in integration
    assert int(re.search(r"#define MP_LIFT_EULER_CONTINUOUS (\d+)", header).group(1)) == lift_ops.EULER_CONTINUOUS == lifting.EULER_CONTINUOUS == 1
    assert lift_ops.EULER_ORDERS == ref.ORDERS == bvh.ORDERS and _lib.ABI_VERSION == 8
    assert manipose_amd.euler_from_rotations is lifting.euler_from_rotations is lift_ops.euler_from_rotations and "euler_from_rotations" in lifting.__all__
    assert lifting.Eulers._fields == ("angles", "pos", "ok")
    source = open(os.path.join(ROOT, "manipose_amd", "csrc", "lift_euler.hip")).read()
    assert "atomicAdd" not in source and "__shared__" not in source and "contract(off)" in source
    for name in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        assert "mp_lift_euler" in open(os.path.join(ROOT, name)).read(), name
    assert "first pass" in open(os.path.join(ROOT, "profiles", "lift", "lift_bvh_bench.txt")).read()
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_euler")
