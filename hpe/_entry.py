"""Shared implementation of the two lifting entry points (counterparts of the reference's Hydra scripts
hpe/main_h36m_lifting.py:711-1270 and hpe/main_3dhp.py:662-1063): same `group.key=value` override grammar, same config
keys (hpe/conf/config.yaml), same model construction (_instantiate_model :613-670), loss assembly (make_loss :101-178),
optimizer / scheduler (:227-270), checkpoint names (save_state :75-98: model{tag}.pth / params{tag}.pth) and the MPJPE
evaluation of evaluate() (hpe/eval_utils.py:16-223: weighted-average, best-score and oracle aggregation, millimetres).
With `data.data_dir` the reference's files (data_3d_h36m.npz + data_2d_h36m_<keypoints>.npz, or data_{train,test}_3dhp.npz) are
ingested on the device (manipose_amd/data/ingest.py) and stay resident in HBM; without it the script trains / evaluates on synthetic
H36M-shaped sequences so that the whole MI355X path (window kernel, engine, fused loss, RCCL data parallelism, fused Adam) runs.
With `run.test` the files of the reference's test pass (main_h36m_lifting.py:840-1186: protocol_1_err.csv, seg_symmetry.csv, seg_consistency.csv,
seg_max_strech.csv, seg_max_delta_strech.csv, cw_err.csv, jw_err.csv, all_seg_errs.npy, all_jw_err_var.npy; main_3dhp.py:769-988: its four single-row
tables) are written into the experiment folder by rank 0 (manipose_amd/report.py); all_pred_hyps.pkl and the mlflow calls are not reproduced.
Launch on N GPUs with `python -m torch.distributed.run --nproc-per-node N hpe/main_h36m_lifting.py ...`.
"""
from __future__ import annotations

import copy
import os
import re
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


from manipose_amd.hydra_lite import Cfg, parse_value  # noqa: E402,F401
from manipose_amd import hydra_lite  # noqa: E402
from manipose_amd.lift_args import is_int_in, is_number  # noqa: E402  (host checks alone: no library, no device)


def load_config(argv, extra_defaults=None):
    """hpe/conf/config.yaml + overrides in the reference's Hydra grammar (main_h36m_lifting.py:711, README.md:54-111): see
    manipose_amd/hydra_lite.py.  Both evaluation commands of the reference's README parse unchanged."""
    return hydra_lite.load_config(os.path.join(ROOT, "hpe", "conf"), argv, extra_defaults)


def instantiate_model(cfg):
    from manipose_amd import ManifoldMixSTE, MixSTE, RMCLManifoldMixSTE, h36m_skeleton
    sk = h36m_skeleton()
    if cfg.model.arch == "mixste":                          # main_h36m_lifting.py:617-628
        model = MixSTE(num_frame=cfg.data.seq_len, num_joints=sk.num_joints, in_chans=2, out_dim=3, num_heads=cfg.model.nheads,
                       depth=cfg.model.layers, embed_dim=cfg.model.channels, drop_path_rate=cfg.model.drop_path_rate, mup=cfg.model.mup)
        model.precision = cfg.model.precision
        _engine_options(model, cfg)
        return model
    kw = dict(skeleton=sk, num_frame=cfg.data.seq_len, num_joints=sk.num_joints, num_bones=sk.num_bones, in_chans=2,
              rot_rep_dim=cfg.model.rot_dim, num_heads_rot=cfg.model.nheads, depth_rot=cfg.model.layers,
              embed_dim_rot=cfg.model.channels, num_heads_seg=cfg.model.nheads_seg, depth_seg=cfg.model.layers_seg,
              embed_dim_seg=cfg.model.channels_seg, drop_path_rate=cfg.model.drop_path_rate, mup=cfg.model.mup)
    if cfg.model.arch == "rmcl_manifold":
        model = RMCLManifoldMixSTE(n_hyp=cfg.multi_hyp.n_hyp, **kw)
    elif cfg.model.arch == "manifold":
        model = ManifoldMixSTE(**kw)
    else:
        raise ValueError(f"Only MixSTE, Manifold-MixSTE and RMCL-Manifold-MixSTE implemented for now. Got option {cfg.model.arch}.")
    model.precision = cfg.model.precision
    _engine_options(model, cfg)
    return model


def _engine_options(model, cfg):
    """model.f16f8 / model.f16_backward of the config (mp_model_config, ABI v7): the operand form of the qkv / fc1 (/ fc2) layers of a
    bf16x3 model (ignored for the other precisions).  Config default since round 6: f16f8 = 3 (all four Linear layers of a block as one fp16 + one
    block-scaled fp8 product; a model that does not qualify runs three bf16 products everywhere), bf16 backward."""
    bf16x3 = str(getattr(cfg.model, "precision", "")) == "bf16x3"
    model.f16f8 = int(getattr(cfg.model, "f16f8", 0)) if bf16x3 else 0
    model.f16_backward = bool(getattr(cfg.model, "f16_backward", False)) if bf16x3 else False


def synthetic_windows(n, T, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    X = (0.3 * torch.randn(n, T, 17, 2, device=device, generator=g)).clamp(-1, 1)
    y = 0.3 * torch.randn(n, T, 17, 3, device=device, generator=g)
    y[:, :, 0] = 0
    return X, y


def synthetic_generator(cfg, device, seed, rank, world):
    """The training data path of the reference (fetch -> PoseSequenceGenerator(random_start=True, PoseFlip(0.5)) -> DataLoader,
    main_h36m_lifting.py:560-610) with the sequences resident in HBM: synthetic H36M-shaped action sequences (no dataset ships here),
    every rank keeps its own shard of them."""
    from manipose_amd import h36m_skeleton
    from manipose_amd.augmentations import PoseFlip
    from manipose_amd.data import PoseSequenceGenerator
    from manipose_amd.distributed import shard_windows
    rng = np.random.default_rng(seed)
    n_seq = max(world, int(cfg.data.get("synthetic_sequences", 16)))
    lens = [int(cfg.data.seq_len) * 4 + 37 * (i % 5) + 11 for i in range(n_seq)]
    mine = list(shard_windows(n_seq, rank, world))
    p3, p2 = [], []
    for i in range(n_seq):
        a = (0.3 * rng.standard_normal((lens[i], 17, 3))).astype(np.float32)
        b = np.clip(0.3 * rng.standard_normal((lens[i], 17, 2)), -1, 1).astype(np.float32)
        a[:, 0] = 0
        if i in mine:
            p3.append(a); p2.append(b)
    tf = PoseFlip(h36m_skeleton(), 0.5) if cfg.train.flip_aug else None
    return PoseSequenceGenerator(p3, p2, None, seq_len=int(cfg.data.seq_len), random_start=True, drop_last=True,
                                 miss_type=cfg.data.get("miss_type", "no_miss"), miss_rate=cfg.data.get("miss_rate", 0.2),
                                 transform=tf, device=device)


def load_sequences(cfg, device):
    """fetch_and_prepare_data + get_subjects_and_actions + the fetch() calls of create_dataloader (main_h36m_lifting.py:511-583,
    main_3dhp.py:503-532): {"train" | "valid": (poses_3d, poses_2d, cameras), "test": {group: (...)}} as lists of device tensors; H36M also
    "test_cams": {group: [the 17 camera numbers fetch() returns per sequence]} (the tuples' third slot stays None: window_generator hands it
    to the generator as its ``actions``).
    The reference's pickle cache of the prepared dataset is not needed: the ingest is a few hundred kernel launches."""
    from manipose_amd.data import Dataset3DHP, Human36mDataset, create_2d_data, fetch, read_3d_data
    from manipose_amd.data.ingest import TEST_SUBJECTS, TRAIN_SUBJECTS
    root = str(cfg.data.data_dir)
    with torch.cuda.device(device):
        if cfg.data.dataset == "3dhp":
            out = {"test": {}}
            if cfg.run.train:
                tr = Dataset3DHP(cfg, root + "/", train=True, device=device)
                out["train"] = (tr.poses, tr.poses_2d, None)
            te = Dataset3DHP(cfg, root + "/", train=False, device=device)
            out["valid"] = (te.poses, te.poses_2d, None)
            out["test"]["all"] = out["valid"]
            return out
        ds = read_3d_data(Human36mDataset(os.path.join(root, f"data_3d_{cfg.data.dataset}.npz"), n_joints=cfg.data.joints, device=device))
        kp = create_2d_data(os.path.join(root, f"data_2d_{cfg.data.dataset}_{cfg.data.keypoints}.npz"), ds)
        if cfg.data.use_valid:
            s_train, s_val = TRAIN_SUBJECTS[:-1], TRAIN_SUBJECTS[-1:]
        else:
            s_train, s_val = TRAIN_SUBJECTS, TEST_SUBJECTS
        if cfg.data.data == "one":
            s_train = [s_train[0]]
        actions = None if cfg.data.actions == "*" else [ds.define_actions(a)[0] for a in str(cfg.data.actions).split(",")]
        have = lambda subjects: [s for s in subjects if s in kp]
        out = {"train": fetch(have(s_train), ds, kp, actions)[:2] + (None,), "valid": fetch(have(s_val), ds, kp, actions)[:2] + (None,), "test": {}, "test_cams": {}}
        for a in (actions or ds.define_actions()):                 # per-action test on S11, main_h36m_lifting.py:884-893
            p3, p2, _, cams = fetch(have(["S11"]), ds, kp, [a])
            if p3:
                out["test"][a] = (p3, p2, None)
                out["test_cams"][a] = cams
        return out


def window_generator(cfg, seqs, train, device):
    """create_dataloader (main_h36m_lifting.py:569-610) minus the DataLoader: the generator itself serves whole batches."""
    from manipose_amd import h36m_skeleton
    from manipose_amd.augmentations import PoseFlip
    from manipose_amd.data import PoseSequenceGenerator
    tf = PoseFlip(h36m_skeleton(), 0.5) if cfg.train.flip_aug else None
    return PoseSequenceGenerator(seqs[0], seqs[1], seqs[2], seq_len=int(cfg.data.seq_len), random_start=train, miss_type=cfg.data.miss_type,
                                 miss_rate=cfg.data.miss_rate, noise_sigma=cfg.data.get("noise_sigma", 5), transform=tf, device=device)


def epoch_batches(gen, batch, shuffle, rank=0, world=1, seed=None, pad=False):
    """DataLoader(shuffle, drop_last=False) over the generator's indices, dealt round-robin over the ranks (DistributedSampler-style:
    every rank draws the same permutation from ``seed`` and keeps every world-th index).  ``pad=True`` (training) wraps the order
    around to a multiple of ``world`` so that every rank runs the same number of steps - each step holds a collective."""
    n = len(gen)
    if shuffle:
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        order = torch.randperm(n, generator=g).tolist()
    else:
        order = list(range(n))
    if pad and world > 1 and n % world:
        order = order + order[:world - n % world]
    order = order[rank::world]
    for i in range(0, len(order), batch):
        yield gen.batch(order[i:i + batch])


def tensor_batches(X, y, batch):
    for i in range(0, X.shape[0], batch):
        yield X[i:i + batch], y[i:i + batch]


@torch.no_grad()
def evaluate(model, X, y=None, batch=None, tta=True, analytics=False, distributed=False, seg_err_samples=0, hypotheses=False):
    """MPJPE (mm) of the aggregated / best-score / oracle hypotheses, with the reference's flip test-time augmentation
    (hpe/eval_utils.py:16-223).  The flipped copy is batched with the original into ONE forward of 2B windows
    instead of a second pass.  ``analytics=True`` adds the reference's evaluation table (main_h36m_lifting.py:933-990,
    main_3dhp.py:860-910: MPSSE, MPSCE, segment-length error, MSE / error variance, 3DPCK, AUC, per-joint errors) of the
    aggregated prediction in millimetres, from the one-pass HIP analytics kernel, and the quantities that are not sums -
    per-bone length extremes, the largest frame-to-frame jump of a bone length, MPJVE, per-coordinate errors, per-joint error variance
    (main_h36m_lifting.py:1044-1089) - with all windows of all batches chained into ONE sequence (mp_bone_extremes).
    ``seg_err_samples`` > 0 also returns ``seg_errs``: that many rows of the per-frame table gt - predicted bone length (mm), drawn like
    the reference's all_seg_errs.npy (:992-1004) from the frames this rank evaluated.  ``distributed=True``: every rank
    evaluates its own share of the batches and the error sums / frame counts are sum-reduced at the end.
    ``hypotheses=True`` adds, for an RMCLManifoldMixSTE only (the key is absent for the other architectures), ``out["hypotheses"]``: the
    multi-hypothesis study of manipose_amd/metrics/hypotheses.py (J-Best, top-m oracle, spread, head usage, score calibration and the
    consistency of the J-Best pose) in millimetres.  It is computed on the hypotheses of the UN-flipped forward - the ones the reference stores
    in all_pred_hyps.pkl (hpe/eval_utils.py:155-160) - also when ``tta`` averages the aggregated predictions with the flipped pass."""
    from manipose_amd import RMCLManifoldMixSTE
    from manipose_amd.augmentations import pose_flip
    from manipose_amd.metrics import mpjpe_error
    from manipose_amd.metrics.analytics import AnalyticsAccumulator, pose_analytics, procrustes_sums
    acc = AnalyticsAccumulator() if analytics else None
    hyp = None
    seg_tables = []
    model.eval()
    sk = model.decoder.skeleton if hasattr(model, "decoder") else _h36m()
    rmcl = isinstance(model, RMCLManifoldMixSTE)
    if hypotheses and rmcl:
        from manipose_amd.metrics.hypotheses import HypothesisAccumulator
        hyp = HypothesisAccumulator()
    sums = {"mpjpe": 0.0, "ps_oracle_mpjpe": 0.0, "oracle_mpjpe": 0.0}
    n = 0
    for xb, yb in (tensor_batches(X, y, batch) if torch.is_tensor(X) else X):      # tensors, or any iterable of (X, y) batches
        nb = xb.shape[0]
        if tta:
            xin = torch.cat([xb, pose_flip((xb.clone(),), sk)[0]], dim=0)
        else:
            xin = xb
        out = model(xin)
        if rmcl:
            poses, scores = out
            pred = model.aggregate(poses[:nb], scores[:nb], "weighted_ave")
            best = model.aggregate(poses[:nb], scores[:nb], "best_score")
            orac = model.aggregate(poses[:nb], mode="oracle", ground_truth=yb)[1]
            if tta:
                hyp_f = pose_flip((poses[nb:].clone(),), sk)[0]          # flipped hypotheses mapped back to the original frame
                pred = (pred + model.aggregate(hyp_f, scores[nb:], "weighted_ave")) / 2
                best = (best + model.aggregate(hyp_f, scores[nb:], "best_score")) / 2
                orac = (orac + model.aggregate(hyp_f, mode="oracle", ground_truth=yb)[1]) / 2
            sums["mpjpe"] += mpjpe_error(pred, yb, "sum").item()
            sums["ps_oracle_mpjpe"] += mpjpe_error(best, yb, "sum").item()
            sums["oracle_mpjpe"] += mpjpe_error(orac, yb, "sum").item()
            if hyp is not None:
                hyp.add(poses[:nb], scores[:nb], yb, pose_scale=1000.0, target_scale=1000.0, consistency=True)
        else:
            pred = out[:nb]
            if tta:
                pred = (pred + pose_flip((out[nb:].clone(),), sk)[0]) / 2
            sums["mpjpe"] += mpjpe_error(pred, yb, "sum").item()
        n += yb.numel() // 3
        if acc is not None:
            acc.add(pose_analytics(pred.detach().contiguous(), yb.contiguous(), pred_scale=1000.0, gt_scale=1000.0))
            acc.add_procrustes(procrustes_sums(pred.detach(), yb, pred_scale=1000.0, gt_scale=1000.0))
            acc.add_extremes(pred.detach().contiguous(), yb.contiguous(), pred_scale=1000.0, gt_scale=1000.0)
            if seg_err_samples > 0:
                from manipose_amd.metrics import segments_len_err
                seg_tables.append(segments_len_err(pred.detach().permute(0, 3, 2, 1), yb.permute(0, 3, 2, 1), sk, mode="no_agg"))
    if distributed:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = torch.tensor([sums["mpjpe"], sums["ps_oracle_mpjpe"], sums["oracle_mpjpe"], float(n)], dtype=torch.float64, device=sk_device(model))
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            sums = {"mpjpe": t[0].item(), "ps_oracle_mpjpe": t[1].item(), "oracle_mpjpe": t[2].item()}
            n = t[3].item()
            if acc is not None:
                acc.all_reduce()
            if hyp is not None:
                hyp.all_reduce()
    out = {k: 1000.0 * v / n for k, v in sums.items() if v > 0}
    if acc is not None:
        out["analytics"] = acc.report()
    if hyp is not None:
        out["hypotheses"] = hyp.report()
    if seg_tables:
        from manipose_amd.report import draw_seg_err_rows
        table = torch.cat(seg_tables, dim=0)
        idx = draw_seg_err_rows(table.shape[0], seg_err_samples)             # the draw on the host, the gather on the device
        out["seg_errs"] = (1000.0 * table[torch.as_tensor(idx, device=table.device)]).cpu().numpy()
    return out


def _h36m():
    from manipose_amd import h36m_skeleton
    return h36m_skeleton()


def sk_device(model):
    return next(model.parameters()).device


LIFT_SUFFIXES = ("__hyps", "__bones", "__traj", "__reproj", "__ok", "__hyps_traj", "__hyps_reproj", "__hyps_ok", "__floor", "__cam", "__traj_fit", "__filled",
                 "__hyps_traj_fit", "__hyps_filled", "__path", "__path_cost", "__steps", "__hyps_steps", "__reproj_smooth", "__hyps_reproj_smooth",
                 "__quat", "__quat_ok", "__hyps_quat", "__hyps_quat_ok", "__root", "__choice", "__spread", "__cost", "__views", "__cam_quat", "__cam_trans",
                 "__cam_rms", "__cam_trans_rms", "__cam_used", "__cam_ok", "__cam_err_deg", "__cam_err_m", "__cam_quat_align", "__cam_trans_align",
                 "__cam_err_deg_align", "__cam_err_m_align", "__cam_bundle_reproj", "__cam_bundle_cost", "__cam_bundle_steps", "__cam_bundle_ok",
                 "__cam_bundle_used", "__tri", "__tri_err", "__tri_views", "__tri_ok", "__tri_steps", "__skel", "__skel_bones", "__skel_err", "__skel_ok",
                 "__skel_steps", "__skel_quat", "__skel_quat_ok", "__skel_err_smooth", "__skel_moves", "__sync_lag", "__sync_contrast", "__sync_used", "__sync_ok",
                 "__sync_curve", "__cal", "__cam_intr", "__cam_focal", "__cam_focal_err", "__cal_reproj", "__cal_cost", "__cal_steps", "__cal_ok", "__cal_used",
                 "__cam_quat_bundle", "__cam_trans_bundle", "__cam_err_deg_bundle", "__cam_err_m_bundle", "__ground_normal", "__ground_offset",
                 "__ground_quat", "__ground_trans", "__ground_rms", "__ground_gap", "__ground_used", "__ground_ok", "__ground_err_deg", "__ground_z",
                 "__contact", "__foot_height", "__skate", "__skate_pairs", "__locked", "__lock_flags", "__lock_moved", "__lock_run", "__skate_locked",
                 "__skate_pairs_locked", "__rt", "__rt_quat", "__rt_root", "__rt_ok", "__rt_taps", "__rt_time", "__rt_fps", "__bvh_euler", "__bvh_pos",
                 "__bvh_ok")


def _scale_and_cost(scale, cost=None, unit="metres"):
    """What the lift.* options check of a scale and, where one goes with it, a cost, each a (key, value): they are numbers, the scale is > 0, the
    cost finite and >= 0.  (That they stay at their defaults while the feature they describe is off is said where the feature is read.)"""
    for key, v in (scale, cost) if cost else (scale,):
        if not is_number(v):
            raise ValueError(f"lift.{key} is a number, got {v!r}")
    if not scale[1] > 0:
        raise ValueError(f"lift.{scale[0]} must be > 0 ({unit}), got {scale[1]!r}")
    if cost and not 0 <= cost[1] < float("inf"):
        raise ValueError(f"lift.{cost[0]} must be finite and >= 0, got {cost[1]!r}")


def lift_place_options(cfg):
    """(place, world, floor) of lift.place / lift.frame / lift.floor; ValueError for a combination that cannot run - before any model is built."""
    place, frame, floor = bool(cfg.lift.get("place", False)), str(cfg.lift.get("frame", "camera")), bool(cfg.lift.get("floor", False))
    if frame not in ("camera", "world"):
        raise ValueError(f"lift.frame must be camera or world, got {frame!r}")
    if floor and frame != "world":
        raise ValueError("lift.floor=true puts the world frame's z on the floor: set lift.frame=world")
    if (place or frame == "world") and str(cfg.data.dataset) == "3dhp":
        raise ValueError("lift.place / lift.frame=world need the cameras' calibration, and the MPI-INF-3DHP files (data.dataset=3dhp) carry none")
    return place, frame == "world", floor


def lift_refine_options(cfg):
    """lift.place_refine as an int: the Gauss-Newton steps after lift.place's linear fit (0: none); ValueError for a value or a combination that
    cannot run - before any model is built."""
    n = cfg.lift.get("place_refine", 0)
    if not is_int_in(n, 0, 16):
        raise ValueError(f"lift.place_refine counts Gauss-Newton steps, an integer in 0..16 (0: off), got {n!r}")
    if n and not bool(cfg.lift.get("place", False)):
        raise ValueError("lift.place_refine refines the trajectory that lift.place fits: set lift.place=true")
    return n


def lift_smooth_options(cfg):
    """(smooth_poses, smooth_traj, smooth_degree, smooth_taper) of the lift group; ValueError for a value or a combination that cannot run - before
    any model is built."""
    radii = []
    for key in ("smooth_poses", "smooth_traj"):
        r = cfg.lift.get(key, 0)
        if not is_int_in(r, 0, 64):
            raise ValueError(f"lift.{key} is a radius in frames, an integer in 0..64 (0: off), got {r!r}")
        radii.append(r)
    degree, taper = cfg.lift.get("smooth_degree", 2), str(cfg.lift.get("smooth_taper", "uniform"))
    if not is_int_in(degree, 0, 2):
        raise ValueError(f"lift.smooth_degree must be 0, 1 or 2, got {degree!r}")
    if taper not in ("uniform", "biweight"):
        raise ValueError(f"lift.smooth_taper must be uniform or biweight, got {taper!r}")
    if not any(radii) and (degree != 2 or taper != "uniform"):
        raise ValueError("lift.smooth_degree / lift.smooth_taper describe smoothing: set lift.smooth_poses or lift.smooth_traj")
    if radii[1] and not bool(cfg.lift.get("place", False)):
        raise ValueError("lift.smooth_traj smooths the trajectory that lift.place fits: set lift.place=true")
    return radii[0], radii[1], degree, taper


def lift_path_options(cfg):
    """(agg, path_sigma, path_switch) of lift.agg / lift.path_sigma / lift.path_switch; ValueError for a value or a combination that cannot run -
    before any model is built."""
    agg = str(cfg.lift.get("agg", "weighted_ave"))
    sigma, switch = cfg.lift.get("path_sigma", 0.02), cfg.lift.get("path_switch", 0.0)
    if agg not in ("weighted_ave", "best_score", "path"):
        raise ValueError(f"lift.agg must be weighted_ave, best_score or path, got {agg!r}")
    _scale_and_cost(("path_sigma", sigma), ("path_switch", switch))
    if agg != "path":
        if sigma != 0.02 or switch != 0.0:
            raise ValueError("lift.path_sigma / lift.path_switch describe the hypothesis path: set lift.agg=path")
        return agg, float(sigma), float(switch)
    if bool(cfg.train.tta):
        raise ValueError("lift.agg=path with train.tta=true: the path runs through the hypotheses of the un-mirrored pass, and head k of a mirrored "
                         "input is not head k of the plain one: set train.tta=false")
    if str(cfg.model.arch) != "rmcl_manifold" or not 2 <= int(cfg.multi_hyp.n_hyp) <= 8:
        raise ValueError("lift.agg=path chooses among a model's hypotheses: it needs model.arch=rmcl_manifold with multi_hyp.n_hyp in 2..8")
    return agg, float(sigma), float(switch)


def lift_score_options(cfg):
    """lift.score as a bool; ValueError for a value or a combination that cannot run - before any model is built."""
    score = cfg.lift.get("score", False)
    if not isinstance(score, bool):
        raise ValueError(f"lift.score must be true or false, got {score!r}")
    if score and not bool(cfg.run.lift):
        raise ValueError("lift.score scores what run.lift lifts: set run.lift=true")
    return score


def lift_rotations_options(cfg):
    """(rotations, continuous) of lift.rotations / lift.rotations_continuous; ValueError for a value or a combination that cannot run - before any
    model is built.  No camera is needed: it works wherever run.lift works."""
    rotations, continuous = cfg.lift.get("rotations", False), cfg.lift.get("rotations_continuous", True)
    if not isinstance(rotations, bool) or not isinstance(continuous, bool):
        raise ValueError(f"lift.rotations and lift.rotations_continuous must be true or false, got {rotations!r}, {continuous!r}")
    if rotations and not bool(cfg.run.lift):
        raise ValueError("lift.rotations computes the joint rotations of what run.lift lifts: set run.lift=true")
    if not continuous and not rotations:
        raise ValueError("lift.rotations_continuous describes the joint rotations: set lift.rotations=true")
    return rotations, continuous


def lift_fuse_options(cfg):
    """(fuse, sigma, score_weight, refine) of lift.fuse / lift.fuse_sigma / lift.fuse_score_weight / lift.fuse_refine; ValueError for a value or a
    combination that cannot run - before any model is built."""
    fuse = cfg.lift.get("fuse", False)
    sigma, weight, refine = cfg.lift.get("fuse_sigma", 0.02), cfg.lift.get("fuse_score_weight", 1.0), cfg.lift.get("fuse_refine", 3)
    if not isinstance(fuse, bool):
        raise ValueError(f"lift.fuse must be true or false, got {fuse!r}")
    _scale_and_cost(("fuse_sigma", sigma), ("fuse_score_weight", weight))
    if not is_int_in(refine, 0, 16):
        raise ValueError(f"lift.fuse_refine counts Gauss-Newton steps, an integer in 0..16, got {refine!r}")
    if not fuse:
        if sigma != 0.02 or weight != 1.0 or refine != 3:
            raise ValueError("lift.fuse_sigma / lift.fuse_score_weight / lift.fuse_refine describe the fusion of a take's views: set lift.fuse=true")
        return False, float(sigma), float(weight), refine
    if not bool(cfg.run.lift):
        raise ValueError("lift.fuse fuses what run.lift lifts: set run.lift=true")
    if str(cfg.data.dataset) == "3dhp":
        raise ValueError("lift.fuse needs the cameras' calibration, and the MPI-INF-3DHP files (data.dataset=3dhp) carry none - nor do they say which "
                         "sequences are one take, so lift.fuse_cameras=estimate cannot help here: cut the takes yourself and give their views' poses to "
                         "manipose_amd.align_views, whose quat and trans are fuse_views' and place_views' extrinsics")
    if bool(cfg.lift.get("keep_padding", False)):
        raise ValueError("lift.fuse with keep_padding: padded frames have no keypoints of their own")
    if bool(cfg.data.data_dir) and (str(cfg.model.arch) != "rmcl_manifold" or not 2 <= int(cfg.multi_hyp.n_hyp) <= 8):
        raise ValueError("lift.fuse chooses among the hypotheses of a take's views: it needs model.arch=rmcl_manifold with multi_hyp.n_hyp in 2..8 "
                         "(a model without hypotheses can be fused only where every take has one view: synthetic-data mode)")
    if int(cfg.multi_hyp.n_hyp) > 8 and str(cfg.model.arch) == "rmcl_manifold":
        raise ValueError("lift.fuse takes at most 8 hypotheses per view: set multi_hyp.n_hyp <= 8")
    return True, float(sigma), float(weight), refine


def lift_fuse_path_options(cfg):
    """(fuse_path, path_sigma, switch_cost) of lift.fuse_path / lift.fuse_path_sigma / lift.fuse_path_switch; ValueError for a value or a
    combination that cannot run - before any model is built."""
    path = cfg.lift.get("fuse_path", False)
    sigma, switch = cfg.lift.get("fuse_path_sigma", 0.02), cfg.lift.get("fuse_path_switch", 0.0)
    if not isinstance(path, bool):
        raise ValueError(f"lift.fuse_path must be true or false, got {path!r}")
    _scale_and_cost(("fuse_path_sigma", sigma), ("fuse_path_switch", switch))
    if not path:
        if sigma != 0.02 or switch != 0.0:
            raise ValueError("lift.fuse_path_sigma / lift.fuse_path_switch describe the path through a take's fused views: set lift.fuse_path=true")
        return False, float(sigma), float(switch)
    if not lift_fuse_options(cfg)[0]:
        raise ValueError("lift.fuse_path chooses the fused views' hypotheses along time: set lift.fuse=true")
    return True, float(sigma), float(switch)


def lift_fuse_align_options(cfg):
    """(estimate, sigma, iters) of lift.fuse_cameras / lift.fuse_align_sigma / lift.fuse_align_iters; ValueError for a value or a combination that
    cannot run - before any model is built."""
    cameras = cfg.lift.get("fuse_cameras", "dataset")
    sigma, iters = cfg.lift.get("fuse_align_sigma", 0.05), cfg.lift.get("fuse_align_iters", 5)
    if cameras not in ("dataset", "estimate"):
        raise ValueError(f"lift.fuse_cameras must be dataset or estimate, got {cameras!r}")
    _scale_and_cost(("fuse_align_sigma", sigma))
    if not is_int_in(iters, 0, 8):
        raise ValueError(f"lift.fuse_align_iters counts re-weightings, an integer in 0..8, got {iters!r}")
    if cameras != "estimate":
        if sigma != 0.05 or iters != 5:
            raise ValueError("lift.fuse_align_sigma / lift.fuse_align_iters describe the estimate of a take's extrinsics: set lift.fuse_cameras=estimate")
        return False, float(sigma), iters
    if not lift_fuse_options(cfg)[0]:
        raise ValueError("lift.fuse_cameras=estimate estimates the extrinsics the fusion uses: set lift.fuse=true")
    return True, float(sigma), iters


def lift_fuse_sync_options(cfg):
    """(estimate, max_lag, min_overlap, sigma, interp) of lift.fuse_sync / lift.fuse_sync_max_lag / lift.fuse_sync_min_overlap / lift.fuse_sync_sigma /
    lift.fuse_sync_interp; ValueError for a value or a combination that cannot run - before any model is built."""
    sync = cfg.lift.get("fuse_sync", "none")
    sync = "none" if sync is None else sync    # (an override lift.fuse_sync=none is read as the null it spells)
    max_lag, overlap = cfg.lift.get("fuse_sync_max_lag", 32), cfg.lift.get("fuse_sync_min_overlap", 16)
    sigma, interp = cfg.lift.get("fuse_sync_sigma", 0.05), cfg.lift.get("fuse_sync_interp", "linear")
    if sync not in ("none", "estimate"):
        raise ValueError(f"lift.fuse_sync must be none or estimate, got {sync!r}")
    if not is_int_in(max_lag, 0, 256):
        raise ValueError(f"lift.fuse_sync_max_lag is the search range in frames, an integer in 0..256, got {max_lag!r}")
    if not is_int_in(overlap, 1, 2 ** 31 - 1):
        raise ValueError(f"lift.fuse_sync_min_overlap counts the pairs of frames a lag needs, an integer >= 1, got {overlap!r}")
    _scale_and_cost(("fuse_sync_sigma", sigma))
    if interp not in ("linear", "nearest"):
        raise ValueError(f"lift.fuse_sync_interp must be linear or nearest, got {interp!r}")
    if sync != "estimate":
        if max_lag != 32 or overlap != 16 or sigma != 0.05 or interp != "linear":
            raise ValueError("lift.fuse_sync_max_lag / lift.fuse_sync_min_overlap / lift.fuse_sync_sigma / lift.fuse_sync_interp describe the estimate of "
                             "the views' lags in time: set lift.fuse_sync=estimate")
        return False, max_lag, overlap, float(sigma), interp
    if not lift_fuse_options(cfg)[0]:
        raise ValueError("lift.fuse_sync=estimate synchronises the views the fusion reads: set lift.fuse=true")
    return True, max_lag, overlap, float(sigma), interp


def lift_fuse_bundle_options(cfg):
    """(steps, sigma) of lift.fuse_bundle / lift.fuse_bundle_sigma; ValueError for a value or a combination that cannot run - before any model is
    built."""
    steps, sigma = cfg.lift.get("fuse_bundle", 0), cfg.lift.get("fuse_bundle_sigma", 0.05)
    if not is_int_in(steps, 0, 8):
        raise ValueError(f"lift.fuse_bundle counts Gauss-Newton steps, an integer in 0..8 (0: off), got {steps!r}")
    _scale_and_cost(("fuse_bundle_sigma", sigma), unit="normalised screen units")
    if steps == 0:
        if sigma != 0.05:
            raise ValueError("lift.fuse_bundle_sigma describes the bundle adjustment of a take's estimated cameras: set lift.fuse_bundle=N, N steps")
        return 0, float(sigma)
    if not lift_fuse_align_options(cfg)[0]:
        raise ValueError("lift.fuse_bundle refines the extrinsics that lift.fuse_cameras=estimate estimates: set lift.fuse_cameras=estimate")
    return steps, float(sigma)


def lift_fuse_calibrate_options(cfg):
    """(steps, sigma, prior, focal, start_focal) of lift.fuse_calibrate / lift.fuse_calibrate_sigma / lift.fuse_calibrate_prior /
    lift.fuse_calibrate_focal / lift.fuse_calibrate_start_focal (0.0: the dataset's intrinsics); ValueError for a value or a combination that
    cannot run - before any model is built."""
    steps, sigma, prior = cfg.lift.get("fuse_calibrate", 0), cfg.lift.get("fuse_calibrate_sigma", 0.05), cfg.lift.get("fuse_calibrate_prior", 0.001)
    focal, start = cfg.lift.get("fuse_calibrate_focal", True), cfg.lift.get("fuse_calibrate_start_focal", 0.0)
    if not is_int_in(steps, 0, 8):
        raise ValueError(f"lift.fuse_calibrate counts Gauss-Newton steps, an integer in 0..8 (0: off), got {steps!r}")
    _scale_and_cost(("fuse_calibrate_sigma", sigma), unit="normalised screen units")
    if not is_number(prior) or not 0 < float(np.float32(prior)) <= float(np.finfo(np.float32).max):
        raise ValueError(f"lift.fuse_calibrate_prior must be a finite number > 0 (the keypoints leave the scale free: the pull towards the fused pose "
                         f"pins it), got {prior!r}")
    if not isinstance(focal, bool):
        raise ValueError(f"lift.fuse_calibrate_focal must be true or false, got {focal!r}")
    if not is_number(start) or not 0 <= float(start) <= float(np.finfo(np.float32).max):
        raise ValueError(f"lift.fuse_calibrate_start_focal is a focal length in normalised screen units, finite and > 0 (0: the dataset's intrinsics), "
                         f"got {start!r}")
    if start > 0 and not lift_fuse_align_options(cfg)[0]:
        raise ValueError("lift.fuse_calibrate_start_focal replaces the intrinsics of a run that estimates its cameras: set lift.fuse_cameras=estimate")
    if steps == 0:
        if sigma != 0.05 or prior != 0.001 or focal is not True:
            raise ValueError("lift.fuse_calibrate_sigma / lift.fuse_calibrate_prior / lift.fuse_calibrate_focal describe the calibration of a take on "
                             "its keypoints: set lift.fuse_calibrate=N, N steps")
        return 0, float(sigma), float(prior), focal, float(start)
    if not lift_fuse_align_options(cfg)[0]:
        raise ValueError("lift.fuse_calibrate refines the cameras that lift.fuse_cameras=estimate estimates: set lift.fuse_cameras=estimate")
    return steps, float(sigma), float(prior), focal, float(start)


def start_focal_cameras(cams, f):
    """lift.fuse_calibrate_start_focal: the cameras with the intrinsics (f, f, 0, 0, 0, 0, 0, 0, 0) - no principal point, no distortion - and their
    own extrinsics and index, as rows of 16 or 17 numbers"""
    from manipose_amd import camera_table
    rows = []
    for cam in cams:
        _, quat, trans = camera_table([cam])
        idx = _camera_index(cam)
        rows.append(np.concatenate([[f, f, 0, 0, 0, 0, 0, 0, 0], quat[0], trans[0], [] if idx is None else [idx]]).astype(np.float32))
    return rows


def lift_fuse_triangulate_options(cfg):
    """(triangulate, steps, sigma, prior) of lift.fuse_triangulate / lift.fuse_triangulate_steps / lift.fuse_triangulate_sigma /
    lift.fuse_triangulate_prior; ValueError for a value or a combination that cannot run - before any model is built."""
    tri, steps = cfg.lift.get("fuse_triangulate", False), cfg.lift.get("fuse_triangulate_steps", 3)
    sigma, prior = cfg.lift.get("fuse_triangulate_sigma", float("inf")), cfg.lift.get("fuse_triangulate_prior", 0.0)
    if not isinstance(tri, bool):
        raise ValueError(f"lift.fuse_triangulate must be true or false, got {tri!r}")
    if not is_int_in(steps, 0, 16):
        raise ValueError(f"lift.fuse_triangulate_steps counts Gauss-Newton steps, an integer in 0..16 (0: the linear start alone), got {steps!r}")
    _scale_and_cost(("fuse_triangulate_sigma", sigma), ("fuse_triangulate_prior", prior), unit="normalised screen units; inf: no robust weight")
    if not tri:
        if steps != 3 or sigma != float("inf") or prior != 0.0:
            raise ValueError("lift.fuse_triangulate_steps / lift.fuse_triangulate_sigma / lift.fuse_triangulate_prior describe the triangulation of a "
                             "fused take's joints: set lift.fuse_triangulate=true")
        return False, steps, float(sigma), float(prior)
    if not lift_fuse_options(cfg)[0]:
        raise ValueError("lift.fuse_triangulate triangulates the joints of a fused take: set lift.fuse=true")
    return True, steps, float(sigma), float(prior)


def lift_fuse_skeleton_options(cfg):
    """(skeleton, steps, sigma, prior) of lift.fuse_skeleton / lift.fuse_skeleton_steps / lift.fuse_skeleton_sigma / lift.fuse_skeleton_prior;
    ValueError for a value or a combination that cannot run - before any model is built."""
    skel, steps = cfg.lift.get("fuse_skeleton", False), cfg.lift.get("fuse_skeleton_steps", 3)
    sigma, prior = cfg.lift.get("fuse_skeleton_sigma", float("inf")), cfg.lift.get("fuse_skeleton_prior", 0.0001)
    if not isinstance(skel, bool):
        raise ValueError(f"lift.fuse_skeleton must be true or false, got {skel!r}")
    if not is_int_in(steps, 0, 16):
        raise ValueError(f"lift.fuse_skeleton_steps counts Gauss-Newton steps, an integer in 0..16 (0: the rigid start alone), got {steps!r}")
    _scale_and_cost(("fuse_skeleton_sigma", sigma), ("fuse_skeleton_prior", prior), unit="normalised screen units; inf: no robust weight")
    if not skel:
        if steps != 3 or sigma != float("inf") or prior != 0.0001:
            raise ValueError("lift.fuse_skeleton_steps / lift.fuse_skeleton_sigma / lift.fuse_skeleton_prior describe the skeleton fit of a fused "
                             "take: set lift.fuse_skeleton=true")
        return False, steps, float(sigma), float(prior)
    if not lift_fuse_options(cfg)[0]:
        raise ValueError("lift.fuse_skeleton fits one skeleton to the keypoints of a fused take: set lift.fuse=true")
    return True, steps, float(sigma), float(prior)


def lift_fuse_skeleton_smooth_options(cfg):
    """(smooth, sweeps) of lift.fuse_skeleton_smooth / lift.fuse_skeleton_sweeps; ValueError for a value or a combination that cannot run - before
    any model is built."""
    smooth, sweeps = cfg.lift.get("fuse_skeleton_smooth", 0.0), cfg.lift.get("fuse_skeleton_sweeps", 8)
    if not is_number(smooth):
        raise ValueError(f"lift.fuse_skeleton_smooth is a number, got {smooth!r}")
    if not 0 <= float(smooth) <= float(np.finfo(np.float32).max):
        raise ValueError(f"lift.fuse_skeleton_smooth must be finite and >= 0 (0: every frame fitted on its own), got {smooth!r}")
    if not is_int_in(sweeps, 0, 64):
        raise ValueError(f"lift.fuse_skeleton_sweeps counts sweeps over a take's frames, an integer in 0..64, got {sweeps!r}")
    if not lift_fuse_skeleton_options(cfg)[0] and (smooth != 0.0 or sweeps != 8):
        raise ValueError("lift.fuse_skeleton_smooth / lift.fuse_skeleton_sweeps describe the skeleton fit of a fused take along time: set "
                         "lift.fuse_skeleton=true")
    return float(smooth), sweeps


GROUND_DEFAULTS = dict(speed=0.01, radius=2, sigma=0.03, prior=0.05, iters=5, foot_height=0.0)      # estimate_ground's own, untuned


def lift_ground_options(cfg):
    """(estimate, kwargs of estimate_ground) of lift.ground / lift.ground_speed / lift.ground_radius / lift.ground_sigma / lift.ground_prior /
    lift.ground_iters / lift.ground_foot_height; ValueError for a value or a combination that cannot run - before any model is built."""
    ground = cfg.lift.get("ground", "none")
    ground = "none" if ground is None else ground      # (an override lift.ground=none is read as the null it spells)
    kw = {k: cfg.lift.get("ground_" + k, v) for k, v in GROUND_DEFAULTS.items()}
    if ground not in ("none", "estimate"):
        raise ValueError(f"lift.ground must be none or estimate, got {ground!r}")
    if not is_int_in(kw["radius"], 1, 8):
        raise ValueError(f"lift.ground_radius is the half width of the speed's central difference in frames, an integer in 1..8, got {kw['radius']!r}")
    if not is_int_in(kw["iters"], 0, 8):
        raise ValueError(f"lift.ground_iters counts the re-weighted solves of the plane, an integer in 0..8, got {kw['iters']!r}")
    if not is_number(kw["speed"]) or not 0 < kw["speed"] < float("inf"):
        raise ValueError(f"lift.ground_speed must be finite and > 0 (metres per frame), got {kw['speed']!r}")
    _scale_and_cost(("ground_sigma", kw["sigma"]), ("ground_prior", kw["prior"]))
    if not is_number(kw["foot_height"]) or not abs(kw["foot_height"]) < float("inf"):
        raise ValueError(f"lift.ground_foot_height must be finite (metres), got {kw['foot_height']!r}")
    if ground != "estimate":
        if any(kw[k] != v for k, v in GROUND_DEFAULTS.items()):
            raise ValueError("lift.ground_speed / lift.ground_radius / lift.ground_sigma / lift.ground_prior / lift.ground_iters / "
                             "lift.ground_foot_height describe the estimate of the floor: set lift.ground=estimate")
        return False, kw
    if not cfg.run.get("lift", False):
        raise ValueError("lift.ground=estimate stands lifted sequences on their floor: set run.lift=true")
    if not lift_fuse_options(cfg)[0] and not lift_place_options(cfg)[0]:
        raise ValueError("lift.ground=estimate reads absolute joint positions: set lift.fuse=true (a take's fused pose at its root) or lift.place=true "
                         "(a sequence's poses at their fitted trajectory)")
    return True, {k: (int(v) if k in ("radius", "iters") else float(v)) for k, v in kw.items()}


FOOTLOCK_DEFAULTS = dict(blend=5, stretch=1.0, floor=True)      # lock_feet's own (floor: the estimated plane is handed over), untuned


def lift_footlock_options(cfg):
    """(lock, kwargs for ground_outputs' ``lock``) of lift.footlock / lift.footlock_blend / lift.footlock_stretch / lift.footlock_floor; ValueError for
    a value or a combination that cannot run - before any model is built."""
    on = cfg.lift.get("footlock", False)
    kw = {k: cfg.lift.get("footlock_" + k, v) for k, v in FOOTLOCK_DEFAULTS.items()}
    if not isinstance(on, bool):
        raise ValueError(f"lift.footlock must be true or false, got {on!r}")
    if not is_int_in(kw["blend"], 0, 32):
        raise ValueError(f"lift.footlock_blend counts the frames of the ease into and out of a stance run, an integer in 0..32, got {kw['blend']!r}")
    if not is_number(kw["stretch"]) or not 0 < kw["stretch"] <= 1:
        raise ValueError(f"lift.footlock_stretch is the share of thigh + shank a leg may reach, a number in (0, 1], got {kw['stretch']!r}")
    if not isinstance(kw["floor"], bool):
        raise ValueError(f"lift.footlock_floor must be true or false, got {kw['floor']!r}")
    if not on:
        if any(kw[k] != v for k, v in FOOTLOCK_DEFAULTS.items()):
            raise ValueError("lift.footlock_blend / lift.footlock_stretch / lift.footlock_floor describe the pinning of the feet: set lift.footlock=true")
        return False, kw
    if not lift_ground_options(cfg)[0]:
        raise ValueError("lift.footlock pins the feet on the contacts of the ground estimate: set lift.ground=estimate")
    return True, dict(blend=int(kw["blend"]), stretch=float(kw["stretch"]), floor=kw["floor"])


RETIME_DEFAULTS = dict(from_fps=0, radius=0, degree=2, taper="uniform")      # retime_rotations' own; from_fps 0: the dataset's frame rate
DATASET_FPS = {"h36m": 50}                  # Human36mDataset.fps; the synthetic sequences are H36M-shaped


def lift_retime_options(cfg):
    """(retime, kwargs for retime_outputs) of lift.retime_fps / lift.retime_from_fps / lift.retime_radius / lift.retime_degree / lift.retime_taper;
    ValueError for a value or a combination that cannot run - before any model is built.  The retimed take is emitted on ONE bone table, so the
    stage needs lift.rotations (what it reads) and lift.rigid (with per-frame lengths there is nothing constant to keep)."""
    fps = cfg.lift.get("retime_fps", 0)
    kw = {k: cfg.lift.get("retime_" + k, v) for k, v in RETIME_DEFAULTS.items()}
    if not is_int_in(fps, 0, 1 << 20):
        raise ValueError(f"lift.retime_fps is the output frame rate, a positive integer (0: off), got {fps!r}")
    if not is_int_in(kw["from_fps"], 0, 1 << 20):
        raise ValueError(f"lift.retime_from_fps is the input frame rate, a positive integer (0: the dataset's), got {kw['from_fps']!r}")
    if not is_int_in(kw["radius"], 0, 64):
        raise ValueError(f"lift.retime_radius must be an integer in 0..64 (0: interpolation), got {kw['radius']!r}")
    if not is_int_in(kw["degree"], 0, 2):
        raise ValueError(f"lift.retime_degree must be 0, 1 or 2, got {kw['degree']!r}")
    if kw["taper"] not in ("uniform", "biweight"):
        raise ValueError(f"lift.retime_taper must be uniform or biweight, got {kw['taper']!r}")
    if fps == 0:
        if any(kw[k] != v for k, v in RETIME_DEFAULTS.items()):
            raise ValueError("lift.retime_from_fps / lift.retime_radius / lift.retime_degree / lift.retime_taper describe the retiming: set lift.retime_fps")
        return False, kw
    if not bool(cfg.run.lift):
        raise ValueError("lift.retime_fps retimes what run.lift lifts: set run.lift=true")
    if not lift_rotations_options(cfg)[0]:
        raise ValueError("lift.retime_fps resamples the joint rotations: set lift.rotations=true")
    if not bool(cfg.lift.get("rigid", False)):
        raise ValueError("lift.retime_fps emits the retimed take on one bone table: set lift.rigid=true (with per-frame lengths there is nothing constant to keep)")
    fps_in = int(kw["from_fps"]) or DATASET_FPS.get(str(cfg.data.dataset), 0)
    if fps_in == 0:
        raise ValueError(f"lift.retime_fps: the frame rate of data.dataset={cfg.data.dataset} is not known here: set lift.retime_from_fps")
    return True, dict(fps_in=fps_in, fps_out=int(fps), radius=int(kw["radius"]), degree=int(kw["degree"]), taper=kw["taper"])


def emitted_triples(out, world):
    """The (root, quat, bones) triples ``out`` holds as they are emitted, what the last stages (lift.retime_fps, lift.bvh) read: a list of
    (key, quat (N, 17, 4), bones (16,), root (N, 3) or None, valid (N,) bool).  Per sequence ``<key>`` with ``__quat`` and ``__bones``: validity
    ``__quat_ok``, the root being ``__traj`` (validity also its ``__filled``, else its ``__ok``) with lift.place in the camera's frame, the poses' own
    joint 0 with lift.frame=world, else none; per fused take ``<key>`` with ``__skel_quat`` and ``__skel_bones``: ``__skel[:, 0]``, validity
    ``__skel_quat_ok`` & ``__skel_ok``."""
    jobs = []
    for k in list(out):
        if k.endswith("__skel_quat") and k[:-len("__skel_quat")] + "__skel_bones" in out:
            key = k[:-len("__skel_quat")]
            jobs.append((key, out[k], out[key + "__skel_bones"], out[key + "__skel"][:, 0], (out[key + "__skel_quat_ok"] != 0) & (out[key + "__skel_ok"] != 0)))
        elif k.endswith("__quat") and k[:-len("__quat")] + "__bones" in out and k[:-len("__quat")] in out:
            key = k[:-len("__quat")]
            valid, root = out[key + "__quat_ok"] != 0, None
            if world:
                root = out[key][:, 0]
            elif key + "__traj" in out:
                root = out[key + "__traj"]
                valid = valid & (out[key + ("__filled" if key + "__filled" in out else "__ok")] != 0)
            jobs.append((key, out[k], out[key + "__bones"], root, valid))
    return jobs


BVH_DEFAULTS = dict(order="ZXY", up="y", scale=100, continuous=True, fps=0)      # fps 0: the dataset's frame rate, or lift.retime_fps
BVH_ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")


def lift_bvh_options(cfg):
    """(bvh, kwargs for bvh_outputs) of lift.bvh / lift.bvh_order / lift.bvh_up / lift.bvh_scale / lift.bvh_continuous / lift.bvh_fps; ValueError
    for a value or a combination that cannot run - before any model is built.  The file holds ONE hierarchy with constant offsets, so the stage
    needs lift.rotations (what it reads) and lift.rigid (the take's one bone table)."""
    on = cfg.lift.get("bvh", False)
    kw = {k: cfg.lift.get("bvh_" + k, v) for k, v in BVH_DEFAULTS.items()}
    if not isinstance(on, bool):
        raise ValueError(f"lift.bvh must be true or false, got {on!r}")
    if kw["order"] not in BVH_ORDERS:
        raise ValueError(f"lift.bvh_order must be one of {', '.join(BVH_ORDERS)}, got {kw['order']!r}")
    if kw["up"] not in ("y", "z"):
        raise ValueError(f"lift.bvh_up is the file's up axis, y or z, got {kw['up']!r}")
    if not is_number(kw["scale"]) or not 0 < float(np.float32(kw["scale"])) < float("inf"):
        raise ValueError(f"lift.bvh_scale is the file's unit, a finite number > 0 (100: centimetres), got {kw['scale']!r}")
    if not isinstance(kw["continuous"], bool):
        raise ValueError(f"lift.bvh_continuous must be true or false, got {kw['continuous']!r}")
    if not is_int_in(kw["fps"], 0, 1 << 20):
        raise ValueError(f"lift.bvh_fps is the file's frame rate, a positive integer (0: the dataset's, or lift.retime_fps), got {kw['fps']!r}")
    if not on:
        if any(kw[k] != v for k, v in BVH_DEFAULTS.items()):
            raise ValueError("lift.bvh_order / lift.bvh_up / lift.bvh_scale / lift.bvh_continuous / lift.bvh_fps describe the export: set lift.bvh=true")
        return False, kw
    if not bool(cfg.run.lift):
        raise ValueError("lift.bvh exports what run.lift lifts: set run.lift=true")
    if not lift_rotations_options(cfg)[0]:
        raise ValueError("lift.bvh writes the joint rotations: set lift.rotations=true")
    if not bool(cfg.lift.get("rigid", False)):
        raise ValueError("lift.bvh writes one hierarchy with constant offsets: set lift.rigid=true (with per-frame lengths there is no bone table)")
    retime_on, retime_kw = lift_retime_options(cfg)
    fps = int(kw["fps"]) or (retime_kw["fps_out"] if retime_on else DATASET_FPS.get(str(cfg.data.dataset), 0))
    if fps == 0:
        raise ValueError(f"lift.bvh: the frame rate of data.dataset={cfg.data.dataset} is not known here: set lift.bvh_fps")
    return True, dict(order=kw["order"], up=kw["up"], scale=float(kw["scale"]), continuous=kw["continuous"], fps=fps, retimed=retime_on)


def bvh_file_name(key):
    """the file of a take or sequence under <experiment>/bvh: its key with everything but letters, digits, '.', '_' and '-' replaced by '_'"""
    return re.sub(r"[^A-Za-z0-9._-]", "_", str(key)) + ".bvh"


def bvh_outputs(out, kw, world, folder):
    """lift.bvh, LAST (after retime_outputs), on what ``out`` holds as it is emitted.  With lift.retime_fps every ``<key>__rt_quat``: (``__rt_root``,
    ``__rt_quat``, the take's bone table, ``__rt_ok`` & 1) at the output rate; otherwise the triples of ``emitted_triples`` at the input's rate.
    Where ``<key>__ground_quat`` exists with ``__ground_ok`` & 1 the take stands on its estimated floor (basis, shift = the ground transform); with
    up = "y" the turn that takes z-up to y-up, (x, y, z) -> (x, z, -y), is composed in front - in float64, rounded once.  euler_from_rotations
    gives ``<key>__bvh_euler`` (M, 17, 3) degrees, ``__bvh_pos`` (M, 3) in the file's unit and ``__bvh_ok`` (M,), and write_bvh
    ``folder/<sanitised key>.bvh`` (none for a take without a frame that has a result).  Returns the files written."""
    from manipose_amd import euler_from_rotations
    from manipose_amd.bvh import write_bvh
    from manipose_amd.data import Skeleton
    from manipose_amd.data.ingest import H36M_JOINT_NAMES_17
    from manipose_amd.data.skeleton import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, H36M_PARENTS, T_POSE_OPERATORS
    sk = Skeleton(list(H36M_PARENTS), list(H36M_JOINTS_LEFT), list(H36M_JOINTS_RIGHT), T_POSE_OPERATORS, joints_names=H36M_JOINT_NAMES_17)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    jobs = []
    for key, quat, bones, root, valid in emitted_triples(out, world):
        if kw["retimed"]:
            quat, root, valid = out[key + "__rt_quat"], out.get(key + "__rt_root"), (out[key + "__rt_ok"] & 1) != 0
        jobs.append((key, quat, bones, root, valid))
    written = []
    for key, quat, bones, root, valid in jobs:
        basis, shift = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
        if key + "__ground_quat" in out and int(out[key + "__ground_ok"]) & 1:
            basis = torch.from_numpy(np.asarray(out[key + "__ground_quat"], np.float64).reshape(4))
            basis = basis / basis.norm()
            shift = torch.from_numpy(np.asarray(out[key + "__ground_trans"], np.float64).reshape(3))
        if kw["up"] == "y":
            basis, shift = bvh_turn_up(basis, shift)
        root = np.zeros((len(quat), 3), np.float32) if root is None else np.asarray(root, np.float32)
        e = euler_from_rotations(up(np.asarray(quat, np.float32)), up(root), up(np.asarray(valid).astype(np.uint8)), None, kw["order"], kw["continuous"],
                                 basis.to(torch.float32), shift.to(torch.float32), kw["scale"])
        angles, pos, ok = e.angles.cpu().numpy(), e.pos.cpu().numpy(), e.ok.cpu().numpy()
        out[key + "__bvh_euler"], out[key + "__bvh_pos"], out[key + "__bvh_ok"] = angles, pos, ok
        path = os.path.join(folder, bvh_file_name(key))
        if not (ok != 0).any():                # (write_bvh would write nothing: no folder is made for it either)
            continue
        os.makedirs(folder, exist_ok=True)
        if write_bvh(path, sk, np.asarray(bones, np.float64), angles, pos, ok, kw["fps"], kw["order"], kw["scale"]):
            written.append(path)
    return written


def bvh_turn_up(basis, shift):
    """(u basis, qrot(u, shift)) in float64 torch tensors, u = (sqrt(1/2), -sqrt(1/2), 0, 0): the quarter turn about x that takes z-up to y-up,
    (x, y, z) -> (x, z, -y), composed in front of p' = qrot(basis, p) + shift"""
    h = float(np.sqrt(0.5))
    w, x, y, z = (float(v) for v in basis.to(torch.float64))
    turned = torch.tensor([h * w + h * x, h * x - h * w, h * y + h * z, h * z - h * y], dtype=torch.float64)      # (h, -h, 0, 0) (w, x, y, z)
    sx, sy, sz = (float(v) for v in shift.to(torch.float64))
    return turned, torch.tensor([sx, sz, -sy], dtype=torch.float64)


def retime_outputs(out, kw, world, targets=None, scores=None):
    """lift.retime_fps, LAST, on what ``out`` holds as it is emitted.  Per sequence ``<key>`` with ``__quat`` and ``__bones``: (root, ``__quat``,
    ``__bones``) with validity ``__quat_ok``, the root being ``__traj`` (validity also its ``__filled``, else its ``__ok``) with lift.place in the
    camera's frame, the poses' own joint 0 with lift.frame=world, else the origin; per fused take ``<key>`` with ``__skel_quat`` and ``__skel_bones``:
    (``__skel[:, 0]``, ``__skel_quat``, ``__skel_bones``) with validity ``__skel_quat_ok`` & ``__skel_ok``.  retime_rotations then pose_from_rotations
    add ``<key>__rt`` (M, 17, 3), the positions in the frame of the poses they come from, ``__rt_quat`` (M, 17, 4), ``__rt_root`` (M, 3) where there is
    a root, ``__rt_ok``, ``__rt_taps`` (M,) uint8, ``__rt_time`` (M,) float64 in input frames and ``__rt_fps`` (2,) int32 (in, out).  ``__locked``, the
    hypotheses and the per-view poses are not retimed.  ``targets`` ({sequence key: (N, 17, 3)}) with equal rates: score_poses' record of ``__rt`` goes
    to ``scores`` (ground truth exists at input frames only: a take retimed to another rate is not scored)."""
    from manipose_amd import pose_from_rotations, retime_rotations, score_poses
    from manipose_amd.lifting import SCORE_FIELDS
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    jobs = emitted_triples(out, world)
    for key, quat, bones, root, valid in jobs:
        r = retime_rotations(up(quat), None if root is None else up(root), up(valid.astype(np.uint8)), None, kw["fps_in"], kw["fps_out"], 0.0, kw["radius"],
                             kw["degree"], kw["taper"])
        poses = pose_from_rotations(r.quat, bones, r.root, r.seq_offset)[0]
        out[key + "__rt"], out[key + "__rt_quat"], out[key + "__rt_ok"] = poses.cpu().numpy(), r.quat.cpu().numpy(), r.ok.cpu().numpy()
        out[key + "__rt_taps"], out[key + "__rt_time"] = r.taps.cpu().numpy(), r.time.cpu().numpy()
        out[key + "__rt_fps"] = np.array([kw["fps_in"], kw["fps_out"]], dtype=np.int32)
        if r.root is not None:
            out[key + "__rt_root"] = r.root.cpu().numpy()
        if targets is not None and scores is not None and key in targets and kw["fps_in"] == kw["fps_out"]:
            rec = score_poses(poses, up(np.asarray(targets[key], dtype=np.float32)), None, (r.ok & 1).contiguous(), root_relative=True)
            scores[key] = {f: getattr(rec, f).cpu().numpy() for f in SCORE_FIELDS}
    return len(jobs)


GROUND_KEYS = ("normal", "offset", "quat", "trans", "rms", "gap", "used", "ok")       # of estimate_ground's record -> "<key>__ground_<k>" in lift.npz


def ground_outputs(out, rows, keys, points, off, valid, up, kw, lock=None, lock_rows=None):
    """lift.ground=estimate on the absolute joint positions ``points`` (Ntot, 17, 3) of the sequences or takes ``keys`` (frames ``off``, ``valid``
    (Ntot) uint8), as they are emitted: estimate_ground's record goes into ``out`` as ``<key>__ground_normal``, ``__ground_offset``, ``__ground_quat``,
    ``__ground_trans``, ``__ground_rms``, ``__ground_gap``, ``__ground_used``, ``__ground_ok``, ``__contact`` (N, 2) uint8, ``__foot_height`` (N, 2),
    ``__skate``, ``__skate_pairs``; held against ``up`` (S, 3), the direction that is up in the frame of the points by the dataset's calibration:
    ``__ground_err_deg``, the angle between the normal and up (NaN without a plane), and ``__ground_z``, the mean of the contact points along up (the
    ankle's height if the dataset's floor is up . x = 0; NaN without a contact).  ``rows`` receives lift_ground.csv's row per key.  The poses are not
    moved: ``__ground_quat`` and ``__ground_trans`` stand them up, to_world's convention.  ``lock`` (lift.footlock: blend, stretch, floor) or None:
    footlock_outputs on the same points, frames and validity, with the contacts and - ``floor`` - the plane estimated here."""
    from manipose_amd import estimate_ground
    g = estimate_ground(points.contiguous(), seq_offset=off, valid=valid.contiguous(), **kw)
    if lock is not None:
        footlock_outputs(out, lock_rows if lock_rows is not None else [], keys, points.contiguous(), off, valid.contiguous(), g, lock)
    host = {k: getattr(g, k).cpu().numpy() for k in g._fields}
    feet = points[:, [3, 6]].cpu().numpy().astype(np.float64)
    for s, key in enumerate(keys):
        sl = slice(int(off[s]), int(off[s + 1]))
        for k in GROUND_KEYS:
            out[f"{key}__ground_{k}"] = host[k][s]
        out[key + "__contact"], out[key + "__foot_height"] = host["contact"][sl], host["height"][sl]
        out[key + "__skate"], out[key + "__skate_pairs"] = host["skate"][s], host["skate_pairs"][s]
        u = np.asarray(up[s], np.float64)
        u = u / np.linalg.norm(u)
        plane, touch = bool(host["ok"][s] & 1), host["contact"][sl] != 0
        err = float(np.degrees(np.arccos(np.clip(host["normal"][s].astype(np.float64) @ u, -1.0, 1.0)))) if plane else float("nan")
        z = float((feet[sl][touch] @ u).mean()) if touch.any() else float("nan")
        out[key + "__ground_err_deg"], out[key + "__ground_z"] = np.float32(err), np.float32(z)
        rows.append(dict(key=key, frames=sl.stop - sl.start, contacts=int(host["used"][s]), rms_mm=1000.0 * float(host["rms"][s]), gap=float(host["gap"][s]),
                         err_deg=err, z_mm=1000.0 * z, skate_mm=1000.0 * float(host["skate"][s]), skate_pairs=int(host["skate_pairs"][s])))


def footlock_outputs(out, rows, keys, points, off, valid, ground, kw):
    """lift.footlock on what ground_outputs estimated the floor from: lock_feet's record goes into ``out`` as ``<key>__locked`` (N, 17, 3), the points
    with the feet pinned, ``__lock_flags`` (N, 2) uint8, ``__lock_moved`` (N, 2), ``__lock_run`` (N, 2) int32, ``__skate_locked`` and
    ``__skate_pairs_locked`` (the skate of ``__locked`` over the contact pairs of ``__contact``: to be read beside ``__skate``); ``rows`` receives
    lift_footlock.csv's row per key.  Nothing that is emitted elsewhere moves."""
    from manipose_amd import lock_feet
    r = lock_feet(points, ground.contact, seq_offset=off, valid=valid, ground=ground if kw["floor"] else None, blend=kw["blend"], stretch=kw["stretch"])
    host = {k: getattr(r, k).cpu().numpy() for k in r._fields}
    before = ground.skate.cpu().numpy()
    for s, key in enumerate(keys):
        sl = slice(int(off[s]), int(off[s + 1]))
        out[key + "__locked"], out[key + "__lock_flags"] = host["points"][sl], host["flags"][sl]
        out[key + "__lock_moved"], out[key + "__lock_run"] = host["moved"][sl], host["run"][sl]
        out[key + "__skate_locked"], out[key + "__skate_pairs_locked"] = host["skate"][s], host["skate_pairs"][s]
        flags, moved = host["flags"][sl], host["moved"][sl].astype(np.float64)
        reached = flags != 0
        rows.append(dict(key=key, frames=sl.stop - sl.start, runs_r=int(host["runs"][s, 0]), runs_l=int(host["runs"][s, 1]), locked=int((flags & 1 != 0).sum()),
                         clamped=int((flags & 4 != 0).sum()), moved_mean_mm=1000.0 * float(moved[reached].mean()) if reached.any() else 0.0,
                         moved_max_mm=1000.0 * float(moved.max()) if moved.size else 0.0, skate_mm=1000.0 * float(before[s]),
                         skate_locked_mm=1000.0 * float(host["skate"][s])))


def write_lift_footlock_report(out_dir, rows):
    """lift_footlock.csv: one row per take or sequence of lift.footlock - runs per foot (right, left), locked and reach-clamped (frame, foot)s, the mean
    (over the feet a pin or an ease reached) and the largest distance an ankle was moved, the skate before and after"""
    path = os.path.join(out_dir, "lift_footlock.csv")
    cols = ("frames", "runs_r", "runs_l", "locked", "clamped", "moved_mean_mm", "moved_max_mm", "skate_mm", "skate_locked_mm")
    with open(path, "w") as f:
        f.write("key," + ",".join(cols) + "\n")
        for r in rows:
            f.write(r["key"] + "," + ",".join(str(r[c]) if isinstance(r[c], int) else f"{r[c]:.6g}" for c in cols) + "\n")
    return path


def write_lift_ground_report(out_dir, rows):
    """lift_ground.csv: one row per take or sequence of lift.ground=estimate"""
    path = os.path.join(out_dir, "lift_ground.csv")
    cols = ("frames", "contacts", "rms_mm", "gap", "err_deg", "z_mm", "skate_mm", "skate_pairs")
    with open(path, "w") as f:
        f.write("key," + ",".join(cols) + "\n")
        for r in rows:
            f.write(r["key"] + "," + ",".join(str(r[c]) if isinstance(r[c], int) else f"{r[c]:.6g}" for c in cols) + "\n")
    return path


def _camera_index(cam):
    """fetch()'s 17th number, a camera dict's "index", or None"""
    if isinstance(cam, dict):
        return cam.get("index")
    a = cam.detach().cpu().numpy() if torch.is_tensor(cam) else np.asarray(cam)
    return float(a[16]) if a.ndim == 1 and a.shape[0] >= 17 else None


def split_takes(cams):
    """The takes of a group: lists of sequence indices; a new take starts wherever the camera index does not increase (a camera without an index:
    a take of its own)."""
    takes, last = [], None
    for i, cam in enumerate(cams):
        idx = _camera_index(cam)
        if not takes or idx is None or last is None or not idx > last:
            takes.append([])
        takes[-1].append(i)
        last = idx
    return takes


def _qrot(q, v):
    """the dataset's camera-to-world rotation of (N, 3) points in float64 (qrot: q is not normalised)"""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    uv = np.cross(np.broadcast_to(q[1:], v.shape), v)
    return v + 2.0 * (q[0] * uv + np.cross(np.broadcast_to(q[1:], v.shape), uv))


CAMERA_KEYS = ("quat", "trans", "rms", "trans_rms", "used", "ok", "err_deg", "err_m")       # of estimate_cameras' dict -> "<fused key>__cam_<k>" in lift.npz
# what lift.fuse_bundle adds to it: the closed form's cameras and their errors, and the bundle's own record
BUNDLE_KEYS = ("quat_align", "trans_align", "err_deg_align", "err_m_align", "bundle_reproj", "bundle_cost", "bundle_steps", "bundle_ok", "bundle_used")


def bundle_cameras(est, cams, takes, bun):
    """lift.fuse_bundle on estimate_cameras' dict, IN PLACE: quat and trans become the bundle's (bundle_views' ViewBundle ``bun``), err_deg and
    err_m are recomputed for them against the dataset's extrinsics, the closed form's values move to ``*_align`` and the bundle's reproj (G, V, 2),
    cost (G, 2), steps, ok (G), used (G, V) are added as ``bundle_*``."""
    from manipose_amd import camera_table
    _, quat, trans = (a.astype(np.float64) for a in camera_table(cams))
    unit = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    for k in ("quat", "trans", "err_deg", "err_m"):
        est[k + "_align"] = est[k].copy()
    est["quat"], est["trans"] = bun.quat.cpu().numpy(), bun.trans.cpu().numpy()
    for t, views in enumerate(takes):
        for v, i in enumerate(views):
            est["err_deg"][t, v], est["err_m"][t, v] = _camera_error(est["quat"][t, v], est["trans"][t, v], unit[i], trans[i])
    for k in ("reproj", "cost", "steps", "ok", "used"):
        est["bundle_" + k] = getattr(bun, k).cpu().numpy()


# what lift.fuse_calibrate adds: the cameras before it (suffix _bundle after lift.fuse_bundle, else _align) and the calibration's own record
CALIBRATE_MOVED = ("quat", "trans", "err_deg", "err_m")
CALIBRATE_KEYS = ("__cal", "__cam_intr", "__cam_focal", "__cam_focal_err", "__cal_reproj", "__cal_cost", "__cal_steps", "__cal_ok", "__cal_used")


def calibrate_cameras(est, cams, true_cams, takes, cal, suffix):
    """lift.fuse_calibrate on estimate_cameras' dict, IN PLACE: quat and trans become the calibration's (calibrate_views' ViewCalibration ``cal``),
    err_deg and err_m are recomputed for them against the dataset's extrinsics, the earlier values move to ``*<suffix>``; intr (G, V, 9), focal
    (G, V, 2): fx at the start and at the end, focal_err (G, V): |fx / the dataset's fx - 1| at the end (``true_cams``: the dataset's cameras,
    ``cams``: the ones the run read), and the calibration's reproj, cost, steps, ok, used are added as ``cal_*``."""
    from manipose_amd import camera_table
    start = camera_table(cams)[0].astype(np.float64)
    true, quat, trans = (a.astype(np.float64) for a in camera_table(true_cams))
    unit = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    for k in CALIBRATE_MOVED:
        est[k + suffix] = est[k].copy()
    est["quat"], est["trans"], est["intr"] = cal.quat.cpu().numpy(), cal.trans.cpu().numpy(), cal.intr.cpu().numpy()
    G, V = est["quat"].shape[:2]
    est["focal"], est["focal_err"] = np.zeros((G, V, 2), np.float32), np.zeros((G, V), np.float32)
    for t, views in enumerate(takes):
        for v, i in enumerate(views):
            est["err_deg"][t, v], est["err_m"][t, v] = _camera_error(est["quat"][t, v], est["trans"][t, v], unit[i], trans[i])
            est["focal"][t, v] = start[i, 0], est["intr"][t, v, 0]
            est["focal_err"][t, v] = abs(float(est["intr"][t, v, 0]) / true[i, 0] - 1.0)
    for k in ("reproj", "cost", "steps", "ok", "used"):
        est["cal_" + k] = getattr(cal, k).cpu().numpy()


def _camera_error(q, t, unit, trans):
    """(degrees, metres) between an estimated camera (q float32 unit, t) and the dataset's (unit quaternion, translation), in float64"""
    q = q.astype(np.float64)
    rel = unit[0] * q[1:] - q[0] * unit[1:] - np.cross(unit[1:], q[1:])                               # the vector part of conj(q_dataset) q
    return np.degrees(2.0 * np.arctan2(np.linalg.norm(rel), abs(float(q @ unit)))), np.linalg.norm(t.astype(np.float64) - trans)


SYNC_KEYS = ("lag", "contrast", "used", "ok", "curve")       # of sync_takes' dict -> "<fused key>__sync_<k>" in lift.npz


def sync_takes(name, res, takes, off, valid, max_lag, min_overlap, sigma, interp):
    """lift.fuse_sync=estimate on one group: every view's lag in time against its take's first view with a usable frame (sync_views on the views'
    merged poses as they were emitted: the signal is each joint's distance from the root, which no camera and no frame of reference changes).  A
    view whose lag could not be estimated keeps lag 0, and so does one whose minimum lies at the border of the search range (the true lag may lie
    outside it); both are reported.  Returns ``(rec, shift)``: rec = {SYNC_KEYS: host arrays (G, V, ..)} as sync_views returned them;
    shift(x, mask=None) = shift_views(x, the lags that are applied, ``mask`` or the takes' own ``valid``, off, interp), which puts a per-view
    array on the take's clock, the reference view's."""
    from manipose_amd import shift_views, sync_views
    V, ftot = int(valid.shape[0]), int(valid.shape[1])
    J, dev = int(res.poses[0].shape[1]), valid.device
    poses = torch.zeros(V, ftot, J, 3, dtype=torch.float32, device=dev)
    for t, views in enumerate(takes):
        for v, i in enumerate(views):
            poses[v, off[t]:off[t + 1]] = res.poses[i]
    got = sync_views(poses, valid, off, max_lag, min_overlap, sigma)
    rec = {k: getattr(got, k).cpu().numpy() for k in SYNC_KEYS}
    applied, lag_int = rec["lag"].copy(), got.lag_int.cpu().numpy()
    for t, views in enumerate(takes):
        for v in range(len(views)):
            if not rec["ok"][t, v] & 1:
                applied[t, v] = 0.0
                print(f"lift.fuse_sync [{name}]: take {t}, view {views[v]}: its lag could not be estimated ({int(rec['used'][t, v])} frames used): "
                      f"the view keeps lag 0", flush=True)
            elif max_lag > 0 and abs(int(lag_int[t, v])) == max_lag:
                applied[t, v] = 0.0
                print(f"lift.fuse_sync [{name}]: take {t}, view {views[v]}: its lag could not be estimated: the minimum lies at the border of the search "
                      f"range (lag {int(lag_int[t, v])}, lift.fuse_sync_max_lag={max_lag}): the view keeps lag 0", flush=True)
    d_lag = torch.from_numpy(applied).to(dev)
    return rec, lambda x, mask=None: shift_views(x, d_lag, valid if mask is None else mask, off, interp)


def estimate_cameras(name, res, seqs, cams, takes, off, hyps, kp, valid, world, refine, sigma, iters, shift=None):
    """lift.fuse_cameras=estimate on one group: every take's extrinsics from its views' merged poses (align_views), the first view's dataset camera
    as the reference - so the world is the dataset's and its z is up.  The views' poses are taken root-relative in their cameras' frames (with
    lift.frame=world they are rotated back, and so are ``hyps``, IN PLACE), every view's root trajectory is fitted on its own (place_poses with the
    view's intrinsics and ``refine`` steps), and the rotation comes from the poses, the translation from the trajectories.  Returns
    ``(est, nested, valid, place_valid)``: est = {CAMERA_KEYS: host arrays (G, V, ..)}, err_deg / err_m the angle and the distance between the
    estimated and the dataset's extrinsics; nested: place_views' cameras with the dataset's intrinsics and the estimated extrinsics; valid without
    the views whose rotation could not be estimated, place_valid also without those whose translation could not.  ``shift`` (sync_takes',
    lift.fuse_sync=estimate; ``hyps``, ``kp`` and ``valid`` are then the UNSHIFTED ones): every view's roots are fitted on its own frames, and the
    merged poses, the roots and their masks are put on the take's clock before align_views reads them; the masks returned are the shifted ones."""
    from manipose_amd import align_views, camera_table, place_poses, to_world
    V, ftot, J, dev, G = int(hyps.shape[0]), int(hyps.shape[1]), int(hyps.shape[3]), hyps.device, len(takes)
    intr, quat, trans = (a.astype(np.float64) for a in camera_table(cams))
    unit = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    back = (unit * np.array([1.0, -1.0, -1.0, -1.0])).astype(np.float32)             # world to camera: the conjugate
    merged = torch.zeros(V, ftot, J, 3, dtype=torch.float32, device=dev)
    table = np.zeros((V, G, 9), np.float32)
    table[..., 0:2] = 1.0
    for t, views in enumerate(takes):
        for v, i in enumerate(views):
            p = res.poses[i].clone()
            if world:
                p = to_world(p, back[i])
                hyps[v, off[t]:off[t + 1]] = to_world(res.hyps[i].clone(), back[i])
            merged[v, off[t]:off[t + 1]] = p - p[:, :1]
            table[v, t] = intr[i]
    starts = np.concatenate([v * ftot + off[:-1] for v in range(V)] + [[V * ftot]]).astype(np.int64)
    traj, _, traj_ok = place_poses(merged.reshape(V * ftot, J, 3), kp.reshape(V * ftot, J, 2), table.reshape(V * G, 9), starts, refine=refine)
    traj, traj_ok = traj.reshape(V, ftot, 3), traj_ok.reshape(V, ftot) & valid
    if shift is not None:                      # lift.fuse_sync=estimate: on the take's clock; a root is there where its fit was ok in the frames it comes from
        merged, valid = shift(merged)
        traj, traj_ok = shift(traj.contiguous(), traj_ok)
    got = align_views(merged, valid, off, traj, traj_ok, sigma, iters, reference=[cams[views[0]] for views in takes])
    est = {k: getattr(got, k).cpu().numpy() for k in CAMERA_KEYS[:6]}
    est["err_deg"], est["err_m"] = np.zeros((G, V), np.float32), np.zeros((G, V), np.float32)
    nested, valid, place_valid = [], valid.clone(), valid.clone()
    for t, views in enumerate(takes):
        row = [None] * V
        for v, i in enumerate(views):
            est["err_deg"][t, v], est["err_m"][t, v] = _camera_error(est["quat"][t, v], est["trans"][t, v], unit[i], trans[i])
            row[v] = np.concatenate([intr[i], est["quat"][t, v], est["trans"][t, v]])
            if not est["ok"][t, v] & 1:
                valid[v, off[t]:off[t + 1]] = 0
                print(f"lift.fuse_cameras [{name}]: take {t}, view {views[v]}: its rotation could not be estimated ({int(est['used'][t, v])} frames used): "
                      f"the view is left out of the take", flush=True)
            if not (est["ok"][t, v] & 2 or v == 0) or not est["ok"][t, v] & 1:
                place_valid[v, off[t]:off[t + 1]] = 0
                if est["ok"][t, v] & 1:
                    print(f"lift.fuse_cameras [{name}]: take {t}, view {views[v]}: its position could not be estimated: the view has no say in the root", flush=True)
        nested.append(row)
    return est, nested, valid, place_valid


def fuse_group(out, name, res, seqs, cams, cfg, targets=None, scores=None, tri_scores=None, skel_scores=None, cal_scores=None, true_cams=None,
               ground_rows=None, footlock_rows=None):
    """lift.fuse on one group: its sequences are cut into takes (split_takes), every take's views are fused (fuse_views: one hypothesis per view,
    chosen jointly; their mean, root-relative in the world's orientation), with lift.rigid re-assembled with the mean of the views' bone tables, and
    placed with ONE world root per frame (place_views); with lift.floor the take stands on z = 0.  ``res``: the group's _Lifted with hypotheses, taken
    after the smoothing and rigid stages.  Writes ``<name>.fused<t>`` and its ``__root``, ``__choice``, ``__spread``, ``__cost``, ``__ok`` (consensus
    and root fit both ok), ``__reproj`` (V, N), ``__steps``, ``__views`` (and ``__floor``) into ``out``; with ``targets`` the take's score into ``scores``.
    With lift.fuse_sync=estimate the views are first synchronised in time (sync_takes: every view's lag against the take's first view, from the merged
    poses, before any camera is estimated) and the hypotheses, the keypoints, the masks and what estimate_cameras reads are put on the first view's
    clock (shift_views, lift.fuse_sync_interp) - the take's clock: the ground truth stays the first view's -; ``__sync_lag``, ``__sync_contrast``,
    ``__sync_used``, ``__sync_ok`` (V,) and ``__sync_curve`` (V, 2 max_lag + 1) are added, as sync_views returned them.
    With lift.fuse_calibrate=N the take is then calibrated on its keypoints (calibrate_views on the fused pose at its placed root, after
    lift.fuse_bundle if that is on, the first view's pose held; calibrate_cameras has the keys), the roots are placed once more and the later
    stages read the new cameras; ``true_cams``: the dataset's cameras where ``cams`` are lift.fuse_calibrate_start_focal's; with ``targets`` the
    calibrated points' score goes into ``cal_scores`` (the frames without a placed root left out).
    With lift.fuse_triangulate every joint is then triangulated on the keypoints (triangulate_views, under the cameras and with the root and ok of the last place_views call) and ``__tri`` (N, 17, 3), in the
    frame of ``<name>.fused<t>``, ``__tri_err``, ``__tri_views``, ``__tri_ok``, ``__tri_steps`` (N, 17) are added; with ``targets`` the triangulated
    pose's score goes into ``tri_scores`` (the frames with a joint whose ok is 0 left out).
    With lift.fuse_skeleton one skeleton is then fitted to the keypoints (fit_skeleton_views, under the same cameras): the start is the
    triangulated point where it has a result and the fused pose plus root elsewhere, a frame is fitted where its root was placed or every joint
    was triangulated, the bone table is the take's lift.rigid table or the start's median; ``__skel`` (N, 17, 3), in the frame of
    ``<name>.fused<t>``, ``__skel_bones`` (16,), ``__skel_err`` (N, 2), ``__skel_ok``, ``__skel_steps`` (N,) and with lift.rotations ``__skel_quat``
    (N, 17, 4), ``__skel_quat_ok`` (N,) are added; with lift.fuse_skeleton_smooth > 0 the take is fitted along time (lift.fuse_skeleton_sweeps
    sweeps): ``__skel``, ``__skel_quat`` and the score are the smoothed fit's, ``__skel_err`` stays (N, 2) and ``__skel_err_smooth`` (N,),
    ``__skel_moves`` (N,) are added; with ``targets`` the fitted pose's score goes into ``skel_scores`` (the frames without a
    result left out).
    With lift.ground=estimate every take's floor is estimated (ground_outputs has the keys) on ``__skel`` where lift.fuse_skeleton is on (the frames
    with a result), else on the fused pose at its root (the frames fused and placed), as emitted - in the dataset's world, so the estimate is held
    against world +z; nothing that is emitted moves.  ``ground_rows`` receives lift_ground.csv's rows; with lift.footlock the feet of the same
    points are pinned (footlock_outputs has the keys) and ``footlock_rows`` receives lift_footlock.csv's."""
    from manipose_amd import (bundle_views, calibrate_views, camera_table, fit_skeleton_views, fuse_views, fuse_views_path, place_views, pose_rotations, project_rigid,
                              score_poses, score_traj, to_world, triangulate_views)
    from manipose_amd.lifting import SCORE_FIELDS
    _, sigma, weight, refine = lift_fuse_options(cfg)
    along, path_sigma, path_switch = lift_fuse_path_options(cfg)
    _, world, floor = lift_place_options(cfg)
    takes = split_takes(cams)
    for t, views in enumerate(takes):
        lens = [int(res.hyps[i].shape[0]) for i in views]
        if len(set(lens)) > 1:
            raise ValueError(f"lift.fuse: the views {views} of take {t} of {name!r} have {lens} frames: the views of a take show the same frames")
        if len(views) > 4:
            raise ValueError(f"lift.fuse: take {t} of {name!r} has {len(views)} views, at most 4 can be fused")
    V, dev = max(len(v) for v in takes), res.hyps[0].device
    if all(len(v) == 1 for v in takes):
        print(f"lift.fuse [{name}]: every take has one view: nothing to agree on, the root is fitted from that view alone", flush=True)
    K, J = int(res.hyps[0].shape[1]), int(res.hyps[0].shape[2])
    frames = [int(res.hyps[v[0]].shape[0]) for v in takes]
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    hyps = torch.zeros(V, int(off[-1]), K, J, 4, dtype=torch.float32, device=dev)
    kp = torch.zeros(V, int(off[-1]), J, 2, dtype=torch.float32, device=dev)
    valid = torch.zeros(V, int(off[-1]), dtype=torch.uint8, device=dev)
    quat = np.zeros((len(takes), V, 4), np.float32)
    quat[..., 0] = 1.0
    for t, views in enumerate(takes):
        for v, i in enumerate(views):
            hyps[v, off[t]:off[t + 1]] = res.hyps[i]
            kp[v, off[t]:off[t + 1]] = torch.as_tensor(seqs[i], dtype=torch.float32).to(dev)
            valid[v, off[t]:off[t + 1]] = 1
            quat[t, v] = camera_table([cams[i]])[1][0]
    nested = [[cams[i] for i in views] + [None] * (V - len(views)) for views in takes]
    estimate, align_sigma, align_iters = lift_fuse_align_options(cfg)
    sync_on, sync_max_lag, sync_overlap, sync_sigma, sync_interp = lift_fuse_sync_options(cfg)
    sync = shift = None
    if sync_on:                                # lift.fuse_sync=estimate: the views' lags in time, before any camera is estimated
        sync, shift = sync_takes(name, res, takes, off, valid, sync_max_lag, sync_overlap, sync_sigma, sync_interp)
    est, q_arg, place_valid = None, None if world else quat, valid
    if estimate:                               # lift.fuse_cameras=estimate: the extrinsics come from the poses, not from the dataset
        est, nested, valid, place_valid = estimate_cameras(name, res, seqs, cams, takes, off, hyps, kp, valid, world, refine, align_sigma, align_iters, shift)
        q_arg = est["quat"]                    # (the hypotheses are back in their cameras' frames)
    if shift is not None:                      # every per-view array the later stages read, on the take's clock (with linear, head k of a frame with
        hyps, moved = shift(hyps)              # head k of the next, scores included: the heads' identity over time is assumed)
        kp = shift(kp)[0]
        if not estimate:
            valid = place_valid = moved
    if along:                                  # lift.fuse_path: the same choice, made jointly over the whole take
        pose, choice, cost, spread, ok, path_cost = fuse_views_path(hyps, q_arg, valid, off, sigma, weight, path_sigma, path_switch)
    else:
        pose, choice, cost, spread, ok = fuse_views(hyps, q_arg, valid, off, sigma, weight)
    tables = None
    if res.bones is not None:                  # lift.rigid: one table per take, the mean of its views'
        tables = torch.stack([torch.stack([res.bones[i] for i in views]).mean(dim=0) for views in takes])
        project_rigid(pose, tables, seq_offset=off)
    root, reproj, placed, steps = place_views(pose, kp, nested, place_valid, off, refine=refine, return_steps=True)
    placed_cams = nested
    bundle_steps, bundle_sigma = lift_fuse_bundle_options(cfg)
    if bundle_steps:                           # lift.fuse_bundle: the estimated cameras and the roots refined jointly on the keypoints, the first view held
        held = np.zeros((len(takes), V), np.uint8)
        held[:, 0] = 1
        bun = bundle_views(pose, root, kp, nested, place_valid, off, placed, held, sigma=bundle_sigma, iters=bundle_steps)
        bundle_cameras(est, cams, takes, bun)
        root, reproj, placed, steps = place_views(pose, kp, bun.cameras, place_valid, off, refine=refine, return_steps=True)
        placed_cams = bun.cameras
    cal_steps, cal_sigma, cal_prior, cal_focal, _ = lift_fuse_calibrate_options(cfg)
    cal = None
    if cal_steps:                              # lift.fuse_calibrate: cameras, focal factors and every joint as a free point, the first view's pose held
        held = np.zeros((len(takes), V), np.uint8)
        held[:, 0] = 1
        cal_in = placed.clone()                # the frames whose start, the fused pose at its placed root, the calibration may use
        cal = calibrate_views((pose + root[:, None]).contiguous(), kp, placed_cams, place_valid, off, placed, held, focal=cal_focal, sigma=cal_sigma,
                              prior=cal_prior, iters=cal_steps)
        calibrate_cameras(est, cams, cams if true_cams is None else true_cams, takes, cal, "_bundle" if bundle_steps else "_align")
        root, reproj, placed, steps = place_views(pose, kp, cal.cameras, place_valid, off, refine=refine, return_steps=True)
        placed_cams = cal.cameras
    tri_on, tri_steps, tri_sigma, tri_prior = lift_fuse_triangulate_options(cfg)
    tri = None
    if tri_on:                                 # lift.fuse_triangulate: every joint on its own, under the cameras and the root of the last placement
        tri = triangulate_views(pose, root, kp, placed_cams, place_valid, off, placed, sigma=tri_sigma, prior=tri_prior, refine=tri_steps)
    skel_on, skel_steps, skel_sigma, skel_prior = lift_fuse_skeleton_options(cfg)
    skel_smooth, skel_sweeps = lift_fuse_skeleton_smooth_options(cfg)
    skel = skel_rot = None
    if skel_on:                                # lift.fuse_skeleton: one body of constant bones per frame, fitted to the keypoints under the same cameras
        start, start_ok = pose + root[:, None], placed
        if tri is not None:
            start = torch.where((tri.ok != 0)[..., None], tri.points, start)
            start_ok = placed | (tri.ok != 0).all(dim=1).to(torch.uint8)
        skel = fit_skeleton_views(start.contiguous(), kp, placed_cams, tables, place_valid, off, start_ok.contiguous(), sigma=skel_sigma,
                                  prior=skel_prior, refine=skel_steps, smooth=skel_smooth, sweeps=skel_sweeps)
        rotations, rot_continuous = lift_rotations_options(cfg)
        if rotations:
            skel_rot = pose_rotations(skel.pose, seq_offset=off, continuous=rot_continuous)
    unit = np.tile(np.array([1, 0, 0, 0], np.float32), (len(takes), 1))
    scene = to_world(pose.clone(), unit, traj=root, seq_offset=off, floor=True if floor else False)
    scene, d_floor = scene if floor else (scene, None)
    ground_on, ground_kw = lift_ground_options(cfg)
    lock_on, lock_kw = lift_footlock_options(cfg)
    if ground_on:                              # lift.ground=estimate: contacts and floor of every take, on the points as they are emitted
        points, known = (skel.pose.clone(), skel.ok & 1) if skel is not None else (pose + root[:, None], ok & placed)
        if floor:
            points[..., 2] -= d_floor.repeat_interleave(torch.as_tensor(frames, device=dev))[:, None]
        ground_outputs(out, ground_rows if ground_rows is not None else [], [f"{name}.fused{t}" for t in range(len(takes))], points, off, known,
                       np.tile(np.array([0.0, 0.0, 1.0]), (len(takes), 1)), ground_kw, lock_kw if lock_on else None, footlock_rows)
    if targets is not None:
        gt_pose, gt_root = [], []
        for views in takes:                    # the first view's ground truth, rotated into the world
            cam = np.concatenate(camera_table([cams[views[0]]]), axis=1)[0].astype(np.float64)
            gt = torch.as_tensor(targets[views[0]]).detach().cpu().numpy().astype(np.float64)
            gt_pose.append(_qrot(cam[9:13], (gt - gt[:, :1]).reshape(-1, 3)).reshape(gt.shape))
            gt_root.append(_qrot(cam[9:13], gt[:, 0]) + cam[13:16])
        d_pose = torch.from_numpy(np.concatenate(gt_pose).astype(np.float32)).to(dev)
        d_root = torch.from_numpy(np.concatenate(gt_root).astype(np.float32)).to(dev)
        rec = score_poses(pose, d_pose, seq_offset=off, root_relative=True)
        ate = score_traj(root, d_root, ok=placed, seq_offset=off)
        if tri is not None:                    # the triangulated pose, made root-relative, against the same ground truth
            tri_rec = score_poses(tri.points, d_pose, seq_offset=off, valid=(tri.ok != 0).all(dim=1).to(torch.uint8), root_relative=True)
            tri_ate = score_traj(tri.points[:, 0].contiguous(), d_root, ok=(tri.ok[:, 0] != 0).to(torch.uint8), seq_offset=off)
        if cal is not None:                    # the calibrated points likewise (the frames the calibration did not use left out)
            cal_rec = score_poses(cal.points, d_pose, seq_offset=off, valid=cal_in, root_relative=True)
            cal_ate = score_traj(cal.points[:, 0].contiguous(), d_root, ok=cal_in, seq_offset=off)
        if skel is not None:                   # the fitted pose likewise
            skel_rec = score_poses(skel.pose, d_pose, seq_offset=off, valid=(skel.ok & 1).contiguous(), root_relative=True)
            skel_ate = score_traj(skel.pose[:, 0].contiguous(), d_root, ok=(skel.ok & 1).contiguous(), seq_offset=off)
    for t, views in enumerate(takes):
        key, sl = f"{name}.fused{t}", slice(int(off[t]), int(off[t + 1]))
        out[key] = scene[sl].cpu().numpy()
        out[key + "__root"], out[key + "__choice"] = root[sl].cpu().numpy(), choice[sl, :len(views)].cpu().numpy()
        out[key + "__spread"], out[key + "__cost"] = spread[sl].cpu().numpy(), cost[sl].cpu().numpy()
        out[key + "__ok"] = (ok[sl] & placed[sl]).cpu().numpy()
        out[key + "__reproj"], out[key + "__steps"] = reproj[:len(views), sl].cpu().numpy(), steps[sl].cpu().numpy()
        out[key + "__views"] = np.array(views, dtype=np.int64)
        if sync is not None:
            for k in SYNC_KEYS:
                out[f"{key}__sync_{k}"] = sync[k][t, :len(views)]
        if est is not None:
            for k in CAMERA_KEYS:
                out[f"{key}__cam_{k}"] = est[k][t, :len(views)]
            for k in BUNDLE_KEYS if bundle_steps else ():
                out[f"{key}__cam_{k}"] = est[k][t, :len(views)] if est[k].ndim > 1 and k != "bundle_cost" else est[k][t]
        if cal is not None:
            for k in CALIBRATE_MOVED:
                out[f"{key}__cam_{k}_{'bundle' if bundle_steps else 'align'}"] = est[k + ("_bundle" if bundle_steps else "_align")][t, :len(views)]
            for k in ("intr", "focal", "focal_err"):
                out[f"{key}__cam_{k}"] = est[k][t, :len(views)]
            points = cal.points[sl].clone()
            if floor:                          # the frame of the fused pose: the same offset off z
                points[..., 2] = points[..., 2] - d_floor[t]
            out[key + "__cal"], out[key + "__cal_reproj"], out[key + "__cal_used"] = points.cpu().numpy(), est["cal_reproj"][t, :len(views)], est["cal_used"][t, :len(views)]
            out[key + "__cal_cost"], out[key + "__cal_steps"], out[key + "__cal_ok"] = est["cal_cost"][t], est["cal_steps"][t], est["cal_ok"][t]
        if along:
            out[key + "__path_cost"] = path_cost[t].cpu().numpy()
        if floor:
            out[key + "__floor"] = d_floor[t].cpu().numpy()
        if tri is not None:
            points = tri.points[sl].clone()
            if floor:                          # the frame of the fused pose: the same offset off z (an item without a result stays 0)
                points[..., 2] = torch.where(tri.ok[sl] != 0, points[..., 2] - d_floor[t], points[..., 2])
            out[key + "__tri"], out[key + "__tri_err"] = points.cpu().numpy(), tri.err[sl].cpu().numpy()
            out[key + "__tri_views"], out[key + "__tri_ok"], out[key + "__tri_steps"] = (v[sl].cpu().numpy() for v in (tri.views, tri.ok, tri.steps))
        if skel is not None:
            fitted = skel.pose[sl].clone()
            if floor:                          # the frame of the fused pose: the same offset off z (a frame without a result stays 0)
                fitted[..., 2] = torch.where((skel.ok[sl] & 1 != 0)[:, None], fitted[..., 2] - d_floor[t], fitted[..., 2])
            out[key + "__skel"], out[key + "__skel_bones"], out[key + "__skel_err"] = fitted.cpu().numpy(), skel.lengths[t].cpu().numpy(), skel.err[sl, :2].cpu().numpy()
            if skel_smooth > 0:                # lift.fuse_skeleton_smooth: __skel is the smoothed fit; its distance and the accepted visits
                out[key + "__skel_err_smooth"], out[key + "__skel_moves"] = skel.err[sl, 2].cpu().numpy(), skel.moves[sl].cpu().numpy()
            out[key + "__skel_ok"], out[key + "__skel_steps"] = skel.ok[sl].cpu().numpy(), skel.steps[sl].cpu().numpy()
            if skel_rot is not None:
                out[key + "__skel_quat"], out[key + "__skel_quat_ok"] = skel_rot[0][sl].cpu().numpy(), skel_rot[1][sl].cpu().numpy()
        if targets is not None and scores is not None:
            scores[key] = {f: getattr(rec, f)[t].cpu().numpy() for f in SCORE_FIELDS}
            scores[key]["traj"] = {"ate": ate.ate[t].cpu().numpy(), "frames": ate.frames[t].cpu().numpy()}
        if targets is not None and tri is not None and tri_scores is not None:
            tri_scores[key] = {f: getattr(tri_rec, f)[t].cpu().numpy() for f in SCORE_FIELDS}
            tri_scores[key]["traj"] = {"ate": tri_ate.ate[t].cpu().numpy(), "frames": tri_ate.frames[t].cpu().numpy()}
        if targets is not None and cal is not None and cal_scores is not None:
            cal_scores[key] = {f: getattr(cal_rec, f)[t].cpu().numpy() for f in SCORE_FIELDS}
            cal_scores[key]["traj"] = {"ate": cal_ate.ate[t].cpu().numpy(), "frames": cal_ate.frames[t].cpu().numpy()}
        if targets is not None and skel is not None and skel_scores is not None:
            skel_scores[key] = {f: getattr(skel_rec, f)[t].cpu().numpy() for f in SCORE_FIELDS}
            skel_scores[key]["traj"] = {"ate": skel_ate.ate[t].cpu().numpy(), "frames": skel_ate.frames[t].cpu().numpy()}


ROTATION_KEYS = {"quat": "__quat", "ok": "__quat_ok", "hyps_quat": "__hyps_quat", "hyps_ok": "__hyps_quat_ok"}      # of a rotations dict -> in lift.npz


def synthetic_cameras(groups):
    """Synthetic-data mode has no calibration of its own: sequence i (in the order of ``groups``) gets camera i % 4 of subject S11 (h36m_cameras())."""
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"]
    cams, i = {}, 0
    for name, seqs in groups.items():
        cams[name] = [s11[(i + k) % 4] for k in range(len(seqs))]
        i += len(seqs)
    return cams


def lift_sequences_to_file(model, cfg, groups, path, cameras=None, targets=None, scores=None, fused_scores=None, tri_scores=None, skel_scores=None,
                           cal_scores=None, ground_rows=None, footlock_rows=None, rt_scores=None):
    """run.lift: one 3-D pose per frame of every sequence of ``groups`` = {name: [poses_2d (N, 17, 2), ...]} (the reference's lift_action,
    hpe/eval_utils.py:226-253, on whole sequences: manipose_amd/lifting.py), written as ONE .npz: key = the group's name (``name.i`` when
    it holds several sequences) -> (N, 17, 3) in metres; with lift.hyps also ``<key>__hyps`` -> (N, K, 17, 4); with lift.rigid (constant bone
    lengths per sequence; lift.lengths, lift.symmetric) also ``<key>__bones`` -> (16,), the sequence's bone lengths in metres.
    ``cameras`` = {name: [one camera per sequence]} (camera_table's forms) is needed by lift.place (also ``<key>__traj`` (N, 3), ``<key>__reproj``
    (N,), ``<key>__ok`` (N,) uint8 and with lift.hyps ``<key>__hyps_traj`` (N, K, 3), ``<key>__hyps_reproj``, ``<key>__hyps_ok`` (N, K); with
    lift.smooth_traj ``__traj`` / ``__hyps_traj`` are the smoothed trajectories and ``<key>__traj_fit`` (N, 3), ``<key>__filled`` (N,) uint8,
    ``<key>__hyps_traj_fit`` (N, K, 3), ``<key>__hyps_filled`` (N, K) are added; with lift.place_refine the trajectories are refined under the full
    camera model and ``<key>__steps`` (N,) uint8, ``<key>__hyps_steps`` (N, K) are added, with lift.smooth_traj also ``<key>__reproj_smooth`` (N,) and
    ``<key>__hyps_reproj_smooth`` (N, K), the reprojection error of the smoothed trajectory) and by
    lift.frame=world (poses and hypotheses in the world frame; with lift.floor on z = 0 and ``<key>__floor``, the offset subtracted); whenever
    cameras were used ``<key>__cam`` holds the 16 numbers (intrinsic 9, orientation 4, translation 3).  With lift.agg=path (one of the model's
    hypotheses per frame, chosen over the whole sequence; lift.path_sigma, lift.path_switch) also ``<key>__path`` (N,) uint8, the hypothesis of
    every frame, and ``<key>__path_cost``, the cost of the sequence's path (a float64 scalar).  With lift.rotations (the joint rotations of the
    poses as emitted, mp_lift_rotations; lift.rotations_continuous) also ``<key>__quat`` (N, 17, 4) float32 unit quaternions (w, x, y, z),
    ``<key>__quat_ok`` (N,) uint8 and with lift.hyps ``<key>__hyps_quat`` (N, K, 17, 4), ``<key>__hyps_quat_ok`` (N, K).
    ``targets`` = {name: [ground truth (N, 17, 3) in metres per sequence]} (lift.score): every sequence is scored against it on the device and the dict
    ``scores`` receives {key: the score dict of lift_sequences(return_score=True) as numpy values, in metres}; the .npz keeps its keys.
    With lift.fuse (``cameras`` needed; lift.fuse_sigma, lift.fuse_score_weight, lift.fuse_refine) the sequences of a group are cut into takes - a
    new take wherever the camera index, fetch()'s 17th number, does not increase - and every take ``t`` also gets ``<name>.fused<t>`` (N, 17, 3), the
    views' consensus pose at ONE world root, with ``__root`` (N, 3), ``__choice`` (N, V) uint8, ``__spread``, ``__cost``, ``__ok``, ``__steps`` (N,),
    ``__reproj`` (V, N), ``__views`` (the sequences' indices within the group), with lift.floor ``__floor`` and with lift.fuse_path (lift.fuse_path_sigma,
    lift.fuse_path_switch) ``__path_cost``, a scalar (fuse_group); with lift.fuse_cameras=estimate (lift.fuse_align_sigma, lift.fuse_align_iters) the
    takes' extrinsics are estimated from the views' poses (estimate_cameras) and ``__cam_quat`` (V, 4), ``__cam_trans`` (V, 3), ``__cam_rms``,
    ``__cam_trans_rms``, ``__cam_used``, ``__cam_ok``, ``__cam_err_deg``, ``__cam_err_m`` (V,) are added, and with lift.fuse_bundle=N
    (lift.fuse_bundle_sigma) they are bundle-adjusted on the keypoints (bundle_views, the first view held; the roots are fitted once more under
    the refined cameras): ``__cam_quat``, ``__cam_trans``, ``__cam_err_deg``, ``__cam_err_m`` are the refined cameras', the closed form's move
    to ``__cam_quat_align``, ``__cam_trans_align``, ``__cam_err_deg_align``, ``__cam_err_m_align``, and ``__cam_bundle_reproj`` (V, 2),
    ``__cam_bundle_cost`` (2,) float64, ``__cam_bundle_steps``, ``__cam_bundle_ok`` (scalars) and ``__cam_bundle_used`` (V,) are added; with ``targets`` the dict
    ``fused_scores`` receives {fused key: score dict} of the fused pose and root against the first view's ground truth in the world.  With
    lift.fuse_sync=estimate (lift.fuse_sync_max_lag, lift.fuse_sync_min_overlap, lift.fuse_sync_sigma, lift.fuse_sync_interp) the views of a take are
    first synchronised in time (sync_takes) and ``__sync_lag``, ``__sync_contrast``, ``__sync_used``, ``__sync_ok`` (V,), ``__sync_curve``
    (V, 2 max_lag + 1) are added.  With
    lift.fuse_triangulate (lift.fuse_triangulate_steps, lift.fuse_triangulate_sigma, lift.fuse_triangulate_prior) every joint of a fused take is
    triangulated on the keypoints of the views that see it (triangulate_views) and ``__tri`` (N, 17, 3), ``__tri_err``, ``__tri_views``, ``__tri_ok``,
    ``__tri_steps`` (N, 17) are added; with ``targets`` the dict ``tri_scores`` receives {fused key: score dict} of the triangulated pose.  With
    lift.fuse_skeleton (lift.fuse_skeleton_steps, lift.fuse_skeleton_sigma, lift.fuse_skeleton_prior) one skeleton of constant bones is fitted to
    the keypoints of every fused take (fit_skeleton_views) and ``__skel`` (N, 17, 3), ``__skel_bones`` (16,), ``__skel_err`` (N, 2), ``__skel_ok``,
    ``__skel_steps`` (N,) and with lift.rotations ``__skel_quat`` (N, 17, 4), ``__skel_quat_ok`` (N,) are added; with ``targets`` the dict
    ``skel_scores`` receives {fused key: score dict} of the fitted pose.  With lift.fuse_calibrate=N (lift.fuse_calibrate_sigma,
    lift.fuse_calibrate_prior, lift.fuse_calibrate_focal; lift.fuse_cameras=estimate needed) every take is then calibrated on its keypoints
    (calibrate_views, after lift.fuse_bundle if that is on: the first view's pose held, every view's focal factor, the other views' poses and every
    joint of the fused pose at its root free), the roots are fitted once more, and triangulation and skeleton fit read the new cameras: ``__cal``
    (N, 17, 3) in the frame of ``<name>.fused<t>``, ``__cam_intr`` (V, 9), ``__cam_focal`` (V, 2): fx at the start and at the end,
    ``__cam_focal_err`` (V,): |fx / the dataset's - 1|, ``__cal_reproj`` (V, 2), ``__cal_cost`` (2,) float64, ``__cal_steps``, ``__cal_ok``,
    ``__cal_used`` (V,) are added; ``__cam_quat``, ``__cam_trans``, ``__cam_err_deg``, ``__cam_err_m`` become the calibrated cameras' and the
    earlier values move to the suffix ``_bundle`` (after lift.fuse_bundle) or ``_align``; with ``targets`` the dict ``cal_scores`` receives {fused
    key: score dict} of the calibrated points.  With lift.fuse_calibrate_start_focal=f every camera the lifting stages read has the intrinsics
    (f, f, 0, 0, 0, 0, 0, 0, 0): the dataset's intrinsics are read for ``__cam_focal_err`` alone.
    With lift.ground=estimate (lift.ground_speed, lift.ground_radius, lift.ground_sigma, lift.ground_prior, lift.ground_iters,
    lift.ground_foot_height; lift.fuse or lift.place needed) the floor under the motion is estimated from the feet that stand still
    (estimate_ground): per fused take with lift.fuse, else per placed sequence on the poses at their trajectory, and ``__ground_normal`` (3,),
    ``__ground_offset``, ``__ground_quat`` (4,), ``__ground_trans`` (3,), ``__ground_rms``, ``__ground_gap``, ``__ground_used``, ``__ground_ok``,
    ``__contact`` (N, 2) uint8, ``__foot_height`` (N, 2), ``__skate``, ``__skate_pairs``, ``__ground_err_deg`` (the angle to the dataset's up: world
    +z, under lift.frame=camera the camera's rotation's) and ``__ground_z`` are added under the take's or the sequence's key; the list ``ground_rows``
    receives a row each for lift_ground.csv.  No emitted pose is moved: ``__ground_quat`` and ``__ground_trans`` stand the take up (to_world).
    With lift.footlock (lift.footlock_blend, lift.footlock_stretch, lift.footlock_floor; lift.ground=estimate needed) the feet of the same points are
    pinned where they stand (lock_feet): ``__locked`` (N, 17, 3), ``__lock_flags``, ``__lock_moved``, ``__lock_run`` (N, 2), ``__skate_locked`` and
    ``__skate_pairs_locked`` are added, and the list ``footlock_rows`` receives a row each for lift_footlock.csv."""
    from manipose_amd import camera_table
    from manipose_amd.lifting import _lift_sequences
    out = {}
    rigid = bool(cfg.lift.get("rigid", False))
    place, world, floor = lift_place_options(cfg)
    smooth_p, smooth_t, smooth_degree, smooth_taper = lift_smooth_options(cfg)
    refine_kw = dict(place_refine=lift_refine_options(cfg)) if lift_refine_options(cfg) else {}
    agg, path_sigma, path_switch = lift_path_options(cfg)
    path_kw = dict(path_sigma=path_sigma, path_switch=path_switch, return_path=True) if agg == "path" else {}
    rotations, rot_continuous = lift_rotations_options(cfg)
    rot_kw = dict(rotations=True, rotations_continuous=rot_continuous, return_rotations=True) if rotations else {}
    use_cams = place or world
    ground_on, ground_kw = lift_ground_options(cfg)
    lock_on, lock_kw = lift_footlock_options(cfg)
    fuse, want_hyps = lift_fuse_options(cfg)[0], bool(cfg.lift.hyps)       # the fusion reads the hypotheses whether or not lift.hyps writes them
    score_kw = lambda name: dict(targets=targets[name], return_score=True) if targets is not None else {}
    to_host = lambda v: {k: to_host(x) for k, x in v.items()} if isinstance(v, dict) else v.cpu().numpy()
    asked = lambda d: d if want_hyps else {k: v for k, v in d.items() if k != "oracle_mpjpe" and not k.startswith("hyps")}
    if use_cams and cameras is None:
        raise ValueError("lift.place / lift.frame=world need the sequences' cameras")
    if fuse and cameras is None:
        raise ValueError("lift.fuse needs the sequences' cameras")
    start_focal, true_cameras = lift_fuse_calibrate_options(cfg)[4], cameras
    if start_focal > 0:                        # lift.fuse_calibrate_start_focal: no stage reads the dataset's intrinsics
        cameras = {name: start_focal_cameras(cams, start_focal) for name, cams in cameras.items()}
    for name, seqs in groups.items():
        res = _lift_sequences(model, seqs, stride=cfg.lift.stride, tta=cfg.train.tta, agg=agg, blend=cfg.lift.blend,
                              return_hyps=want_hyps or fuse, batch=cfg.train.batch_size_test, rigid=rigid, lengths=cfg.lift.get("lengths", None),
                              symmetric=bool(cfg.lift.get("symmetric", False)), return_bones=rigid, cameras=cameras[name] if use_cams else None,
                              place=place, frame="world" if world else "camera", floor=floor, return_place=place or floor,
                              smooth_poses=smooth_p, smooth_traj=smooth_t, smooth_degree=smooth_degree, smooth_taper=smooth_taper, **refine_kw, **path_kw, **rot_kw, **score_kw(name))
        cam_rows = np.concatenate(camera_table(cameras[name]), axis=1) if use_cams else None
        for i, p in enumerate(res.poses):
            key = name if len(res.poses) == 1 else f"{name}.{i}"
            out[key] = p.cpu().numpy()
            if res.hyps is not None and want_hyps:
                out[key + "__hyps"] = res.hyps[i].cpu().numpy()
            if res.bones is not None:
                out[key + "__bones"] = res.bones[i].cpu().numpy()
            if res.place is not None:
                for k, v in asked(res.place[i]).items():
                    out[f"{key}__{k}"] = v.cpu().numpy()
            if cam_rows is not None:
                out[key + "__cam"] = cam_rows[i]
            if res.path is not None:
                out[key + "__path"], out[key + "__path_cost"] = (v.cpu().numpy() for v in res.path[i])
            if res.rotations is not None:
                for k, v in asked(res.rotations[i]).items():
                    out[key + ROTATION_KEYS[k]] = v.cpu().numpy()
            if res.score is not None and scores is not None:
                scores[key] = to_host(asked(res.score[i]))
        if fuse:
            fuse_group(out, name, res, seqs, cameras[name], cfg, targets[name] if targets is not None else None, fused_scores, tri_scores, skel_scores,
                       cal_scores, true_cameras[name], ground_rows, footlock_rows)
        elif ground_on:                        # lift.ground=estimate on placed sequences: the poses at their trajectory, in the frame they are emitted in
            keys = [name if len(res.poses) == 1 else f"{name}.{i}" for i in range(len(res.poses))]
            points = torch.cat([p if world else p + res.place[i]["traj"][:, None] for i, p in enumerate(res.poses)])
            known = torch.cat([res.place[i]["ok"] for i in range(len(res.poses))])
            off = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in res.poses])]).astype(np.int64)
            up = [np.array([0.0, 0.0, 1.0]) if world else _qrot(cam_rows[i][9:13] * np.array([1, -1, -1, -1]), np.array([[0.0, 0.0, 1.0]]))[0]
                  for i in range(len(res.poses))]      # world +z; in a camera's frame its rotation's up, R^T z
            ground_outputs(out, ground_rows if ground_rows is not None else [], keys, points, off, known, up, ground_kw, lock_kw if lock_on else None, footlock_rows)
    retime_on, retime_kw = lift_retime_options(cfg)
    if retime_on:                              # lift.retime_fps: last, on what is emitted (retime_outputs has the keys)
        by_key = None
        if targets is not None:
            by_key = {(name if len(seqs) == 1 else f"{name}.{i}"): t for name, seqs in groups.items() for i, t in enumerate(targets[name])}
        retime_outputs(out, retime_kw, world, by_key, rt_scores)
    bvh_on, bvh_kw = lift_bvh_options(cfg)
    if bvh_on:                                 # lift.bvh: the very last, on what is emitted (bvh_outputs has the keys and the files)
        bvh_files = bvh_outputs(out, bvh_kw, world, os.path.join(os.path.dirname(os.path.abspath(path)), "bvh"))
        print(f"lift.bvh: {len(bvh_files)} files at {bvh_kw['fps']} fps, channels {bvh_kw['order']}, {bvh_kw['up']} up -> {os.path.dirname(bvh_files[0]) if bvh_files else 'none'}",
              flush=True)
    np.savez(path, **out)
    return out


def synthetic_sequences_2d(cfg, seed):
    """The 2-D side of the synthetic H36M-shaped action sequences (synthetic_generator), one group per sequence."""
    rng = np.random.default_rng(seed)
    n_seq = int(cfg.data.get("synthetic_sequences", 16))
    lens = [int(cfg.data.seq_len) * 4 + 37 * (i % 5) + 11 for i in range(n_seq)]
    return {f"synthetic_{i:03d}": [np.clip(0.3 * rng.standard_normal((n, 17, 2)), -1, 1).astype(np.float32)] for i, n in enumerate(lens)}


def synthetic_sequences_3d(cfg, seed):
    """The 3-D side of synthetic_sequences_2d, in the form fetch() prepares ground truth (joint 0: the root's position in the camera's frame, a few
    metres in front of it; the other joints relative to the root).  It draws from a generator stream of its own, so the 2-D sequences keep their bits."""
    rng = np.random.default_rng([int(seed), 3])
    n_seq = int(cfg.data.get("synthetic_sequences", 16))
    lens = [int(cfg.data.seq_len) * 4 + 37 * (i % 5) + 11 for i in range(n_seq)]
    out = {}
    for i, n in enumerate(lens):
        a = (0.3 * rng.standard_normal((n, 17, 3))).astype(np.float32)
        a[:, 0, 2] += np.float32(4.0)
        out[f"synthetic_{i:03d}"] = [a]
    return out


def save_state(model, trainer, scheduler_state, epoch, folder, tag=None):
    tag = f"_{tag}" if tag else ""
    torch.save(model.state_dict(), os.path.join(folder, f"model{tag}.pth"))
    torch.save({"optimizer": trainer.opt.state_dict(), "scheduler": scheduler_state, "epoch": epoch},
               os.path.join(folder, f"params{tag}.pth"))


def run(argv, extra_defaults=None):
    from manipose_amd.distributed import broadcast_parameters, init_from_env
    from manipose_amd.training import LiftingTrainer
    cfg = load_config(argv, extra_defaults)
    lift_place_options(cfg)                    # a lift.place / lift.frame / lift.floor that cannot run fails here, before the model is built
    lift_smooth_options(cfg)                   # ... and so does a lift.smooth_* that cannot run
    lift_refine_options(cfg)                   # ... and a lift.place_refine without lift.place
    lift_path_options(cfg)                     # ... and a lift.agg=path that cannot (with the default train.tta=true: set train.tta=false)
    lift_score_options(cfg)                    # ... and a lift.score without run.lift
    lift_rotations_options(cfg)                # ... and a lift.rotations without run.lift
    lift_fuse_options(cfg)                     # ... and a lift.fuse without run.lift, without calibration or without hypotheses
    lift_fuse_path_options(cfg)                # ... and a lift.fuse_path without lift.fuse
    lift_fuse_align_options(cfg)               # ... and a lift.fuse_cameras=estimate without lift.fuse
    lift_fuse_bundle_options(cfg)              # ... and a lift.fuse_bundle without lift.fuse_cameras=estimate
    lift_fuse_calibrate_options(cfg)           # ... and a lift.fuse_calibrate without lift.fuse_cameras=estimate
    lift_fuse_sync_options(cfg)                # ... and a lift.fuse_sync=estimate without lift.fuse
    lift_fuse_triangulate_options(cfg)         # ... and a lift.fuse_triangulate without lift.fuse
    lift_fuse_skeleton_options(cfg)            # ... and a lift.fuse_skeleton without lift.fuse
    lift_fuse_skeleton_smooth_options(cfg)     # ... and a lift.fuse_skeleton_smooth without lift.fuse_skeleton
    lift_ground_options(cfg)                   # ... and a lift.ground=estimate with neither lift.fuse nor lift.place
    lift_footlock_options(cfg)                 # ... and a lift.footlock without lift.ground=estimate
    lift_retime_options(cfg)                   # ... and a lift.retime_fps without run.lift, lift.rotations or lift.rigid
    lift_bvh_options(cfg)                      # ... and a lift.bvh without them, or a bvh option without lift.bvh
    rank, world, local = init_from_env()
    if not torch.cuda.is_available():
        raise RuntimeError("the lifting entry points need an MI355X (ROCm device); there is no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    torch.manual_seed(cfg.run.seed)
    model = instantiate_model(cfg)
    mup_mults = None
    if cfg.model.mup:                          # create_model / set_mup_base_shapes (main_h36m_lifting.py:673-708): BEFORE any checkpoint is loaded,
        # as in the reference - set_base_shapes rescales the freshly initialised MuReadout weights by sqrt(width_mult), which must never
        # touch weights that come from a checkpoint
        from manipose_amd.mup_lite import make_base_shapes, mu_init_params, mup_lr_multipliers, set_base_shapes
        small, big = copy.deepcopy(cfg), copy.deepcopy(cfg)
        small["model"]["channels"], small["model"]["channels_seg"], small["data"]["seq_len"] = 64, 64, 27
        big["model"]["channels"], big["model"]["channels_seg"], big["data"]["seq_len"] = 128, 128, 81
        set_base_shapes(model, make_base_shapes(instantiate_model(Cfg.wrap(small)), instantiate_model(Cfg.wrap(big))))
        mup_mults = mup_lr_multipliers(model)
    if cfg.run.checkpoint_model:               # main_h36m_lifting.py:754-760: checkpoint weights are used untouched
        ck = torch.load(cfg.run.checkpoint_model, map_location="cpu")
        model.load_state_dict(ck["model_pos"] if "model_pos" in ck else ck)
    elif cfg.model.mup:                        # :761-764: re-initialisation according to muP only without a checkpoint
        mu_init_params(model)
    model.max_batch_hint = max(cfg.train.batch_size, 2 * cfg.train.batch_size_test)      # x2: flip-TTA batches the mirrored copy
    model = model.to(dev)
    if cfg.train.get("lat_sym_regularization", 0) > 0:
        print("warning: Lateral symmetry regularization is not implemented yet!", flush=True)      # as main_h36m_lifting.py:109-110
    trainer = LiftingTrainer(model, lr=cfg.train.lr, weight_decay=1e-6, w_loss=cfg.train.w_loss, vel_loss=cfg.train.vel_loss,
                             smooth_reg=cfg.train.smooth_reg, rmcl_score_reg=cfg.train.rmcl_score_reg, seed=cfg.run.seed,
                             sq_loss=cfg.train.sq_loss, rigid_seg_reg=cfg.train.get("rigid_seg_reg", 0.0))
    if mup_mults is not None:                  # MuAdam (main_h36m_lifting.py:227-232): matrix-like parameters train with lr / width_mult
        trainer.opt.set_multipliers(mup_mults)
    broadcast_parameters(model.flat_parameters())
    start_epoch, sched_state = 0, None
    if cfg.run.checkpoint_params:
        st = torch.load(cfg.run.checkpoint_params, map_location="cpu")
        trainer.opt.load_state_dict(st["optimizer"])
        trainer.step_no = trainer.opt.step_count          # DropPath masks are a function of (seed, step): continue, do not replay
        start_epoch = st["epoch"]
        sched_state = st.get("scheduler")
    T, B, Bt = cfg.data.seq_len, cfg.train.batch_size, cfg.train.batch_size_test
    out_dir = os.path.join(os.getcwd(), cfg.run.experiment)
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
    real = bool(cfg.data.data_dir)
    # evaluation is sharded over the ranks like training whenever every rank gets at least one window; the error sums and
    # frame counts are sum-reduced inside evaluate(); otherwise rank 0 evaluates alone
    def sharded(gen):
        share = world > 1 and len(gen) >= world
        return (lambda: epoch_batches(gen, Bt, shuffle=False, rank=rank if share else 0, world=world if share else 1)), share

    def allsum(v):
        t = torch.tensor([v], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t)
        return t.item()

    if real:
        seqs = load_sequences(cfg, dev)
        gen_valid = window_generator(cfg, seqs["valid"], False, dev)
        valid_batches, valid_shared = sharded(gen_valid)
        if rank == 0:
            print(f">>> Validation dataset length: {len(gen_valid)} windows of {T} frames", flush=True)
    else:
        Xv, yv = synthetic_windows(4 * Bt, T, dev, seed=10_000)
        valid_shared = world > 1 and Xv.shape[0] >= world
        valid_batches = (lambda: tensor_batches(Xv[rank::world], yv[rank::world], Bt)) if valid_shared else (lambda: tensor_batches(Xv, yv, Bt))
    from manipose_amd.optim import make_lr_scheduler
    sched = make_lr_scheduler(trainer.opt, cfg.train.lr_scheduler, cfg.train.epochs, cfg.train.n_annealing, cfg.train.lr_min,
                              cfg.train.lr_patience, cfg.train.lr_threshold)            # main_h36m_lifting.py:243-264
    if sched_state is not None and sched_state.get("kind") == sched.state_dict()["kind"]:
        sched.load_state_dict(sched_state)
    best_val, best_eval = 1e10, {}
    best_model_state = None                  # main_h36m_lifting.py:390,491: weights of the best validation loss / best MPJPE, reloaded before the test
    train_curve, valid_curve = [], []
    if cfg.run.train:
        if real:
            gen = window_generator(cfg, seqs["train"], True, dev)       # sequences resident in HBM, one gather kernel per batch
            if rank == 0:
                print(f">>> Training dataset length: {len(gen)} windows of {T} frames", flush=True)
        else:
            gen = synthetic_generator(cfg, dev, cfg.run.seed, rank, world)
        torch.manual_seed(cfg.run.seed + 1000 * rank)                        # per-rank window / flip draws
        np.random.seed(cfg.run.seed + 1000 * rank)                           # per-rank occlusion draws
        for epoch in range(start_epoch, cfg.train.epochs):
            model.train()
            acc = torch.zeros(4, device=dev)
            if real:       # one pass over the windows, shuffled, dealt over the ranks (main_h36m_lifting.py:597-610)
                batches = epoch_batches(gen, B, shuffle=True, rank=rank, world=world, seed=cfg.run.seed + epoch, pad=True)
            else:          # shuffled sampling with replacement over this rank's synthetic windows
                batches = (gen.batch(torch.randint(0, len(gen), (B,)).tolist()) for _ in range(cfg.train.steps_per_epoch))
            steps = 0
            for X, y in batches:
                acc += trainer.train_step(X, y)                      # device-side accumulation: no per-step host sync
                steps += 1
            terms = (acc / max(steps, 1)).tolist()
            train_curve.append(sum(terms))
            if (epoch + 1) % cfg.train.valid_epoch_interval == 0:
                model.eval()
                val = sum(trainer.eval_loss(xb, yb).sum().item() for xb, yb in valid_batches())
                if valid_shared:
                    val = allsum(val)
                valid_curve.append(val)
                if best_val > val:                                     # main_h36m_lifting.py:374-398
                    best_val = val
                    best_model_state = copy.deepcopy(model.state_dict())
                    if rank == 0:
                        save_state(model, trainer, sched.state_dict(), epoch, out_dir, "best_val")
                if cfg.train.lr_scheduler == "plateau":                # :400-403: the plateau scheduler watches the running best
                    sched.step(best_val)
                else:
                    sched.step()
            if rank == 0:
                names = ("wloss", "score_reg", "vloss", "sreg") if trainer.rmcl else ("wloss", "vloss", "sreg", "rigid_seg_reg")
                print(f"epoch {epoch}: tr_loss {sum(terms):.5f} " + " ".join(f"{n} {v:.5f}" for n, v in zip(names, terms))
                      + f" | best val {best_val:.5f} lr {sched.get_last_lr()[0]:.2e}", flush=True)
            if (epoch + 1) % cfg.train.mpjpe_epoch_interval == 0 and (rank == 0 or valid_shared):      # main_h36m_lifting.py:405-470
                ev = evaluate(model, valid_batches(), tta=cfg.train.tta, distributed=valid_shared)
                if rank == 0:
                    print("   eval:", {k: round(v, 3) for k, v in ev.items()}, flush=True)
                for key, tag in (("mpjpe", "best_mpjpe"), ("oracle_mpjpe", "best_oracle_mpjpe"), ("ps_oracle_mpjpe", "best_ps_oracle_mpjpe")):
                    if key in ev and ev[key] < best_eval.get(key, 1e10):           # tags of main_h36m_lifting.py:440-489
                        best_eval[key] = ev[key]
                        if key == "mpjpe":
                            best_model_state = copy.deepcopy(model.state_dict())
                        if rank == 0:
                            save_state(model, trainer, sched.state_dict(), epoch, out_dir, tag)
        if rank == 0:
            save_state(model, trainer, sched.state_dict(), cfg.train.epochs, out_dir, "end")
            np.save(os.path.join(out_dir, "train_loss.npy"), np.array(train_curve))           # :503-504
            np.save(os.path.join(out_dir, "valid_loss.npy"), np.array(valid_curve))
        if best_model_state is not None:                   # "load best weights" (main_h36m_lifting.py:506-507): the test below runs on them
            model.load_state_dict(best_model_state)
    if cfg.run.test:
        groups = {"synthetic": (valid_batches, valid_shared)}
        if real:        # per action (H36M: subject S11, main_h36m_lifting.py:884-990) or the whole 3DHP test set (main_3dhp.py:800-910)
            groups = {name: sharded(window_generator(cfg, sq, False, dev)) for name, sq in seqs["test"].items()}
        from manipose_amd import report
        rows, reports, hyps = {}, {}, {}
        want_hyps = bool(cfg.run.get("hyp_report", False))
        for name, (make, shared) in groups.items():
            if rank != 0 and not shared:
                continue
            res = evaluate(model, make(), tta=cfg.train.tta, analytics=True, distributed=shared, seg_err_samples=report.SEG_ERR_SAMPLES,
                           hypotheses=want_hyps)
            table = res.pop("analytics")
            if "hypotheses" in res:
                hyps[name] = res.pop("hypotheses")
            reports[name] = dict(res, analytics=table)
            res.pop("seg_errs", None)
            rows[name] = res
            if rank == 0:
                print(f"test [{name}]:", {k: round(v, 3) for k, v in res.items()}, flush=True)
                print(f"test analytics [{name}] (mm):", {k: round(v, 4) for k, v in table.items() if not isinstance(v, list)}, flush=True)
        if len(rows) > 1 and rank == 0:
            keys = sorted({k for r in rows.values() for k in r})
            print("test [average over groups]:", {k: round(float(np.mean([r[k] for r in rows.values() if k in r])), 3) for k in keys}, flush=True)
        if rank == 0 and reports:              # the files behind the paper's tables (main_h36m_lifting.py:1158-1186, main_3dhp.py:978-988)
            if real and cfg.data.dataset == "3dhp":
                written = report.write_3dhp_report(out_dir, next(iter(reports.values()))["analytics"])
            else:
                from manipose_amd import RMCLManifoldMixSTE
                written = report.write_h36m_report(out_dir, reports, rmcl=isinstance(model, RMCLManifoldMixSTE))
            if hyps:                           # run.hyp_report: the hypothesis study, one row per group (3DHP: single-row tables)
                written += report.write_hypothesis_report(out_dir, hyps, single=real and cfg.data.dataset == "3dhp")
            print(f"report: {len(written)} files -> {out_dir}", flush=True)
    if cfg.run.lift and rank == 0:         # after run.checkpoint_model / the training above: the weights the test ran on
        groups = {name: sq[1] for name, sq in seqs["test"].items()} if real else synthetic_sequences_2d(cfg, cfg.run.seed)
        path = cfg.lift.output if os.path.isabs(str(cfg.lift.output)) else os.path.join(out_dir, str(cfg.lift.output))
        cams = None
        if any(lift_place_options(cfg)[:2]) or lift_fuse_options(cfg)[0]:
            cams = seqs["test_cams"] if real else synthetic_cameras(groups)
        targets, scores, fused_scores, tri_scores, skel_scores, cal_scores = None, {}, {}, {}, {}, {}
        if lift_score_options(cfg):            # the 3-D ground truth beside the 2-D sequences that are lifted
            targets = {name: sq[0] for name, sq in seqs["test"].items()} if real else synthetic_sequences_3d(cfg, cfg.run.seed)
        ground_rows, footlock_rows, rt_scores = [], [], {}
        lifted = lift_sequences_to_file(model, cfg, groups, path, cams, targets, scores, fused_scores, tri_scores, skel_scores, cal_scores, ground_rows,
                                        footlock_rows, rt_scores)
        if lift_retime_options(cfg)[0]:
            kw = lift_retime_options(cfg)[1]
            print(f"lift.retime: {sum(1 for k in lifted if k.endswith('__rt'))} takes or sequences from {kw['fps_in']} to {kw['fps_out']} fps, radius {kw['radius']}",
                  flush=True)
        if lift_ground_options(cfg)[0]:
            print(f"lift.ground: {len(ground_rows)} floors estimated -> {write_lift_ground_report(out_dir, ground_rows)}", flush=True)
        if lift_footlock_options(cfg)[0]:
            print(f"lift.footlock: feet pinned in {len(footlock_rows)} takes or sequences -> {write_lift_footlock_report(out_dir, footlock_rows)}", flush=True)
        is_pose = lambda k: not k.endswith(LIFT_SUFFIXES) and ".fused" not in k
        print(f"lift: {sum(v.shape[0] for k, v in lifted.items() if is_pose(k))} frames of {len(groups)} groups -> {path}", flush=True)
        if lift_fuse_options(cfg)[0]:
            takes = [k for k in lifted if ".fused" in k and not k.endswith(LIFT_SUFFIXES)]
            print(f"lift.fuse: {len(takes)} takes fused, {sum(lifted[k].shape[0] for k in takes)} frames", flush=True)
        if targets is not None:
            from manipose_amd import report
            written = report.write_lift_score_report(out_dir, scores)
            n = np.array([float(v["frames"]) for v in scores.values()])
            mean = lambda key: 1000.0 * float(np.nansum(n * np.array([float(v[key]) for v in scores.values()])) / max(1.0, n.sum()))
            print(f"lift score (mm, {int(n.sum())} frames of {len(scores)} sequences): mpjpe {mean('mpjpe'):.3f}, p-mpjpe {mean('p_mpjpe'):.3f}, "
                  f"mpjve {mean('mpjve'):.3f}, accel {mean('accel'):.3f} -> {written[0]}", flush=True)
            if rt_scores:                      # lift.retime_fps at the input's rate: rotation-space smoothing, scored at the input's frames
                print(f"lift score, retimed sequences -> {report.write_lift_score_report(out_dir, rt_scores, name='lift_score_rt', joints=False)[0]}", flush=True)
            if fused_scores:
                print(f"lift score, fused takes -> {report.write_lift_score_report(out_dir, fused_scores, name='lift_score_fused', joints=False)[0]}",
                      flush=True)
            if tri_scores:
                print(f"lift score, triangulated takes -> {report.write_lift_score_report(out_dir, tri_scores, name='lift_score_tri', joints=False)[0]}",
                      flush=True)
            if cal_scores:
                print(f"lift score, calibrated takes -> {report.write_lift_score_report(out_dir, cal_scores, name='lift_score_cal', joints=False)[0]}",
                      flush=True)
            if skel_scores:
                print(f"lift score, fitted skeletons -> {report.write_lift_score_report(out_dir, skel_scores, name='lift_score_skel', joints=False)[0]}",
                      flush=True)
    return best_val
