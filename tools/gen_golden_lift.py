"""Generates tests/golden/lift.npz by running the reference's own ``lift_action`` (hpe/eval_utils.py:226-253) on a tiny seeded rMCL
model: 3 sequences of lengths < T, = 2 T and 2 T + 5 through its PoseSequenceGenerator(drop_last=False) and a DataLoader, flip-TTA
on, with and without ``return_hyps``.  Data only (weights, inputs, the reference's outputs).

    python tools/gen_golden_lift.py          (where oracle/gen_golden.py finds the reference)

The reference is imported at run time under the stand-ins of oracle/gen_golden.py (timm's DropPath, mup.MuReadout); eval_utils.py
also imports ``omegaconf`` for one type annotation, which gets an empty stand-in here when the package is absent."""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden  # noqa: E402
import manipose_ref as orc  # noqa: E402

CFG = dict(T=9, J=17, num_bones=16, C_rot=32, depth_rot=2, heads_rot=4, C_seg=16, depth_seg=1, heads_seg=4, n_hyp=3)   # the size of rmcl_tiny
CFG_KEYS = ("T", "J", "num_bones", "C_rot", "depth_rot", "heads_rot", "C_seg", "depth_seg", "heads_seg", "n_hyp")
LENGTHS = (5, 18, 23)


def main():
    ref = gen_golden.import_reference()           # (also puts the reference's hpe/ folder on sys.path)
    try:
        import omegaconf  # noqa: F401
    except ImportError:
        om = types.ModuleType("omegaconf")
        om.DictConfig = dict
        sys.modules["omegaconf"] = om
    import eval_utils
    from mh_so3_hpe.data.generators import PoseSequenceGenerator
    from torch.utils.data import DataLoader
    torch.manual_seed(5)
    st = orc.make_state(CFG, seed=5)
    model = gen_golden.build_ref_model(ref, CFG, 0.0)
    model.load_state_dict(st, strict=True)
    model.eval()
    g = np.random.default_rng(31)
    p2 = [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in LENGTHS]
    out = {"cfg": np.array([CFG[k] for k in CFG_KEYS], dtype=np.int64), "lens": np.array(LENGTHS, dtype=np.int64)}
    out.update(gen_golden.np_state(st))
    for i, a in enumerate(p2):
        out[f"p2.{i}"] = a
    config = types.SimpleNamespace(train=types.SimpleNamespace(tta=True))
    for key, hyps in (("lift", False), ("lift_hyps", True)):
        # float64 copies: the reference's flip works in place on views of float32 dataset arrays
        a2 = [a.astype(np.float64) for a in p2]
        a3 = [np.zeros((a.shape[0], 17, 3)) for a in p2]
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            gen = PoseSequenceGenerator(a3, a2, None, seq_len=CFG["T"], random_start=False, drop_last=False, miss_type="no_miss")
            loader = DataLoader(gen, batch_size=2, shuffle=False, num_workers=0)
            res = eval_utils.lift_action(loader, model, "cpu", config, ref["sk"], hyps)
        out[key] = np.asarray(res, dtype=np.float32)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "lift.npz"), **out)
    print("lift: ok", {k: out[k].shape for k in ("lift", "lift_hyps")})


if __name__ == "__main__":
    main()
