"""The multi-hypothesis study on the GPU (C ABI ``mp_hypothesis_stats``, manipose_amd/csrc/hypothesis_stats.hip): what the reference
computes on the host from its dump of every hypothesis (all_pred_hyps.pkl) - ``calc_jbest_mpjpe`` / ``calc_jbest_pose``
(hpe/useful_aux_scripts/eval_baselines.py:451-481), the consistency of the J-Best pose (:425-440), the per-joint spread of the hypotheses
(inspect_multimodality.py) and the error against the number of hypotheses (plot_nhyps_lineplot.py) - plus what tells whether the scoring
head is calibrated and whether heads are dead.  One pass over hypotheses that are already resident on the device.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .. import _lib

NJ, KMAX = 17, 8
# float row of mp_hypothesis_stats (include/manipose_hip.h)
F_FRAMES, F_BEST, F_ORACLE, F_JBEST, F_WAVE, F_S_ORACLE, F_S_MAX, F_PAIR, F_TOPM, F_JB_JOINT, F_SPREAD, F_MASS, NF = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 33, 50, 58
# count row
C_AGREE, C_ORANK, C_PBEST, C_SHEAD, C_JHEAD, NI = 0, 1, 9, 17, 25, 33


@dataclass
class HypothesisStats:
    """The two rows of ``mp_hypothesis_stats`` for one batch, on the device: sums over its B*T frames."""
    sums: torch.Tensor                     # (row_floats,) float32
    counts: torch.Tensor                   # (row_counts,) int64
    B: int
    K: int
    T: int
    jbest_pose: Optional[torch.Tensor] = None      # (B, T, 17, 3): per joint the hypothesis closest to the target, the input's bits
    jbest_idx: Optional[torch.Tensor] = None       # (B, T, 17) uint8: which one

    @property
    def frames(self) -> int:
        return self.B * self.T


def _check(poses, scores, target):
    if poses.device.type != "cuda":
        raise RuntimeError("manipose_amd: the hypothesis study runs on the ROCm device only (HIP kernel, no CPU fallback)")
    if poses.dim() != 5 or poses.shape[-2:] != (NJ, 3):
        raise AssertionError(f"expected hypotheses of shape (B, K, T, {NJ}, 3), got {tuple(poses.shape)}")
    B, K, T = poses.shape[:3]
    if not 1 <= K <= KMAX:
        raise AssertionError(f"1 to {KMAX} hypotheses are supported, got {K}")
    if tuple(scores.shape) != (B, K, T) and tuple(scores.shape) != (B, K, T, 1):
        raise AssertionError(f"expected scores of shape (B, K, T), got {tuple(scores.shape)}")
    if tuple(target.shape) != (B, T, NJ, 3):
        raise AssertionError(f"expected a target of shape (B, T, {NJ}, 3), got {tuple(target.shape)}")
    return B, K, T


def hypothesis_stats(poses: torch.Tensor, scores: torch.Tensor, target: torch.Tensor, pose_scale: float = 1.0, target_scale: float = 1.0,
                     return_jbest: bool = False) -> HypothesisStats:
    """poses (B, K, T, 17, 3), scores (B, K, T), target (B, T, 17, 3) on the device -> ``HypothesisStats``.  Errors are those of
    ``pose_scale * poses`` against ``target_scale * target``; ``return_jbest`` also fills ``jbest_pose`` (unscaled) and ``jbest_idx``."""
    B, K, T = _check(poses, scores, target)
    dev = poses.device
    p = poses.detach().float().contiguous()
    s = scores.detach().to(dev).float().reshape(B, K, T).contiguous()
    g = target.detach().to(dev).float().contiguous()
    lib = _lib.load()
    sums = torch.empty(int(lib.mp_hypothesis_stats_row_floats()), device=dev)
    counts = torch.empty(int(lib.mp_hypothesis_stats_row_counts()), dtype=torch.int64, device=dev)
    jp = torch.empty(B, T, NJ, 3, device=dev) if return_jbest else None
    ji = torch.empty(B, T, NJ, dtype=torch.uint8, device=dev) if return_jbest else None
    scratch = torch.empty(int(lib.mp_hypothesis_stats_scratch_floats(B * T)), device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mp_hypothesis_stats(_lib.ptr(p), _lib.ptr(s), _lib.ptr(g), B, K, T, float(pose_scale), float(target_scale),
                                           _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(jp), _lib.ptr(ji), _lib.ptr(scratch), scratch.numel(),
                                           _lib.stream_ptr()), "mp_hypothesis_stats")
    return HypothesisStats(sums, counts, B, K, T, jp, ji)


def _uniform_scores(predicted: torch.Tensor) -> torch.Tensor:
    B, H, L = predicted.shape[:3]
    return torch.full((B, H, L), 1.0 / H, device=predicted.device)


def calc_jbest_mpjpe(predicted: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """eval_baselines.py:451-457: predicted (B, H, L, J, D), target (B, L, J, D) -> mean over (B, L, J) of the smallest per-joint error
    over the H hypotheses (0-dim tensor on the device)."""
    st = hypothesis_stats(predicted, _uniform_scores(predicted), target)
    return st.sums[F_JBEST] / float(st.frames * NJ)


def calc_jbest_pose(predicted: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """eval_baselines.py:460-481: (B, L, J, D), per joint the coordinates of the hypothesis closest to the target (the first of equals)."""
    return hypothesis_stats(predicted, _uniform_scores(predicted), target, return_jbest=True).jbest_pose


class HypothesisAccumulator:
    """Adds up ``hypothesis_stats`` rows over evaluation batches in float64 / int64 and reports the study.  Every quantity is a sum over
    frames, so ``all_reduce`` is a plain SUM over the ranks - nothing here is local to a rank."""

    def __init__(self):
        self.sums: Optional[torch.Tensor] = None        # (NF,) float64
        self.counts: Optional[torch.Tensor] = None      # (NI,) int64
        self.K = 0
        self.consistency = None                         # AnalyticsAccumulator of the J-Best poses (add(consistency=True))

    def add_stats(self, st: HypothesisStats) -> None:
        if self.sums is None:
            self.sums, self.counts, self.K = st.sums.double().clone(), st.counts.clone(), st.K
        else:
            if st.K != self.K:
                raise AssertionError(f"batches of {self.K} and of {st.K} hypotheses cannot be added")
            self.sums += st.sums.double()
            self.counts += st.counts

    def add(self, poses: torch.Tensor, scores: torch.Tensor, target: torch.Tensor, pose_scale: float = 1.0, target_scale: float = 1.0,
            consistency: bool = False) -> HypothesisStats:
        """One batch.  ``consistency=True`` also feeds the J-Best pose to ``pose_analytics`` (MPSSE / MPSCE of the J-Best pose, the
        d3dp_jbest_* quantities of eval_baselines.py:432-435)."""
        st = hypothesis_stats(poses, scores, target, pose_scale, target_scale, return_jbest=consistency)
        self.add_stats(st)
        if consistency:
            from .analytics import AnalyticsAccumulator, pose_analytics
            if self.consistency is None:
                self.consistency = AnalyticsAccumulator()
            self.consistency.add(pose_analytics(st.jbest_pose, target.detach().to(st.jbest_pose.device).float().contiguous(),
                                                pred_scale=pose_scale, gt_scale=target_scale))
        return st

    def all_reduce(self, group=None) -> None:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        if self.sums is None:
            raise RuntimeError("HypothesisAccumulator.all_reduce: every rank must have added at least one batch")
        dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)
        if self.consistency is not None:
            self.consistency.all_reduce(group)

    def report(self) -> dict:
        if self.sums is None:
            raise RuntimeError("HypothesisAccumulator.report: nothing was added")
        s, c, K = self.sums.cpu(), self.counts.cpu(), self.K
        n = float(s[F_FRAMES])
        nj = n * NJ
        share = lambda o: (c[o:o + K].double() / n).tolist()
        out = {"mpjpe_weighted_ave": (s[F_WAVE] / nj).item(), "mpjpe_best_score": (s[F_BEST] / nj).item(),
               "mpjpe_oracle": (s[F_ORACLE] / nj).item(), "mpjpe_jbest": (s[F_JBEST] / nj).item(),
               "mpjpe_top_m": (s[F_TOPM:F_TOPM + K] / nj).tolist(),
               "jbest_per_joint": (s[F_JB_JOINT:F_JB_JOINT + NJ] / n).tolist(), "spread_per_joint": (s[F_SPREAD:F_SPREAD + NJ] / n).tolist(),
               "pairwise_distance": (s[F_PAIR] / nj).item(),
               "score_of_oracle": (s[F_S_ORACLE] / n).item(), "score_max": (s[F_S_MAX] / n).item(), "top1_agreement": c[C_AGREE].item() / n,
               "oracle_rank_hist": share(C_ORANK), "pbest_head_share": share(C_PBEST), "score_head_share": share(C_SHEAD),
               "jbest_head_share": (c[C_JHEAD:C_JHEAD + K].double() / nj).tolist(), "score_mass_per_head": (s[F_MASS:F_MASS + K] / n).tolist()}
        if self.consistency is not None:
            t = self.consistency.report()
            out["jbest_mpsse"], out["jbest_mpsce"] = t["mpsse"], t["mpsce"]
        return out
