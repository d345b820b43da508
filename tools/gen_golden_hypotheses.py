"""Generates tests/golden/hypotheses.npz by running the reference's own multi-hypothesis evaluation on seeded hypotheses in millimetres:
``calc_jbest_mpjpe`` / ``calc_jbest_pose`` (hpe/useful_aux_scripts/eval_baselines.py:451-481) and ``RMCLManifoldMixSTE.aggregate`` in its
modes ``oracle`` / ``best_score`` / ``weighted_ave`` (architectures/rmcl_manifold_mix_ste.py:141-185) followed by ``mpjpe_error``.  Data only.

    python tools/gen_golden_hypotheses.py          (where oracle/gen_golden.py finds the reference)

eval_baselines.py cannot be imported - it is a notebook-style script that runs at top level on files of its author's machine - so the two
function definitions are taken out of its syntax tree and compiled in memory; nothing of them is written anywhere.

Input sets (B, K, L) = (2, 5, 9) and (1, 8, 40): hypothesis = target + unit direction x (20 + 12 q + 4.4 r) mm, q a per-(frame, joint)
permutation of 0..K-1 and r a per-frame one, all on a 1/4 mm grid (exact in float32; the file stays below 100 KB).  Asserted here in float64:
per joint the two smallest distances differ by more than 0.1 mm and any two pose errors of a frame by more than 0.1 mm, no two scores of a
frame are equal - no arg-min / arg-max hangs on rounding."""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden  # noqa: E402

SETS = ((2, 5, 9), (1, 8, 40))
TINY = dict(T=9, J=17, num_bones=16, C_rot=32, depth_rot=1, heads_rot=4, C_seg=16, depth_seg=1, heads_seg=4, n_hyp=5)


def reference_jbest():
    """calc_jbest_mpjpe, calc_jbest_pose of the reference, compiled from the two FunctionDef nodes of its script."""
    import mh_so3_hpe                                         # importable once gen_golden.import_reference() has run
    path = os.path.join(os.path.dirname(os.path.abspath(list(mh_so3_hpe.__path__)[0])), "useful_aux_scripts", "eval_baselines.py")
    tree = ast.parse(open(path).read())
    wanted = ("calc_jbest_mpjpe", "calc_jbest_pose")
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(d.name for d in defs) == sorted(wanted)
    from einops import rearrange
    ns = {"torch": torch, "rearrange": rearrange}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns["calc_jbest_mpjpe"], ns["calc_jbest_pose"]


def make_set(B, K, L, seed):
    g = np.random.default_rng(seed)
    gt = 250.0 * g.standard_normal((1, 1, 17, 3)) + 2.0 * np.cumsum(g.standard_normal((B, L, 17, 3)), axis=1)
    gt[:, :, 0] = 0.0
    gt = np.round(4.0 * gt) / 4.0
    d = g.standard_normal((B, K, L, 17, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    q = np.argsort(g.random((B, L, 17, K)), -1).transpose(0, 3, 1, 2)
    r = np.argsort(g.random((B, L, K)), -1).transpose(0, 2, 1)[..., None]
    hyp = np.round(4.0 * (gt[:, None] + d * (20.0 + 12.0 * q + 4.4 * r)[..., None])) / 4.0
    s = g.random((B, K, L)) + 0.05
    s = (s / s.sum(1, keepdims=True)).astype(np.float32)
    hyp, gt = hyp.astype(np.float32), gt.astype(np.float32)
    e = np.sqrt(((hyp.astype(np.float64) - gt.astype(np.float64)[:, None]) ** 2).sum(-1))          # (B, K, L, 17)
    es = np.sort(e, axis=1)
    E = np.sort(e.sum(-1), axis=1)
    assert (es[:, 1] - es[:, 0]).min() > 0.1 and np.diff(E, axis=1).min() > 0.1 and np.diff(np.sort(s, axis=1), axis=1).min() > 0, (B, K, L)
    return hyp, s, gt


def main():
    ref = gen_golden.import_reference()
    M = ref["M"]
    jbest_mpjpe, jbest_pose = reference_jbest()
    model = gen_golden.build_ref_model(ref, TINY, 0.0)        # aggregate() uses no weight: any RMCLManifoldMixSTE serves
    out = {"sets": np.array(SETS, dtype=np.int64)}
    for i, (B, K, L) in enumerate(SETS):
        hyp, s, gt = make_set(B, K, L, seed=60 + i)
        h, sc, y = torch.from_numpy(hyp), torch.from_numpy(s)[..., None], torch.from_numpy(gt)      # scores (B, K, L, 1) as the model returns them
        out[f"hyp.{i}"], out[f"scores.{i}"], out[f"gt.{i}"] = hyp, s, gt
        out[f"jbest_mpjpe.{i}"] = np.float32(jbest_mpjpe(h, y).item())
        out[f"jbest_pose.{i}"] = jbest_pose(h, y).numpy()
        with torch.no_grad():
            orac = model.aggregate(h, mode="oracle", ground_truth=y)[1]
            best = model.aggregate(h, sc, "best_score")
            wave = model.aggregate(h, sc, "weighted_ave")
        for key, p in (("oracle", orac), ("best_score", best), ("weighted_ave", wave)):
            out[f"mpjpe_{key}.{i}"] = np.float32(M.mpjpe_error(p, y, "average").item())
    path = os.path.join(ROOT, "tests", "golden", "hypotheses.npz")
    np.savez_compressed(path, **out)
    print("hypotheses: ok", os.path.getsize(path), "bytes", {k: float(v) for k, v in out.items() if k.startswith(("jbest_mpjpe", "mpjpe_"))})


if __name__ == "__main__":
    main()
