"""What the GPU tests of sequence lifting share (test_gpu_lift.py, test_gpu_lift_rigid.py, test_gpu_lift_place.py): the tiny fp32 fixture
models, built once per process, their synthetic input sequences, and the bit-for-bit comparison."""
import numpy as np

from helpers import fixture_state, load_fixture

FIXTURES = {"rmcl": "rmcl_small", "manifold": "manifold_k1", "mixste": "mixste_tiny"}
_MODELS = {}


def fixture_model(kind):
    """(model on the device in eval mode, T, K) of the fixture FIXTURES[kind]"""
    if kind in _MODELS:
        return _MODELS[kind]
    from manipose_amd import ManifoldMixSTE, MixSTE, RMCLManifoldMixSTE, h36m_skeleton
    fx = load_fixture(FIXTURES[kind])
    if kind == "mixste":
        T, C_, depth, heads = [int(v) for v in fx["cfg_mixste"]]
        model = MixSTE(num_frame=T, num_joints=17, in_chans=2, out_dim=3, embed_dim=C_, depth=depth, num_heads=heads, drop_path_rate=0.0)
        K = 1
    else:
        c = fx["cfg"]
        kw = dict(skeleton=h36m_skeleton(), num_frame=c["T"], embed_dim_rot=c["C_rot"], depth_rot=c["depth_rot"], num_heads_rot=c["heads_rot"],
                  embed_dim_seg=c["C_seg"], depth_seg=c["depth_seg"], num_heads_seg=c["heads_seg"], drop_path_rate=0.0, rot_rep_dim=c.get("rot_dim", 6))
        model = RMCLManifoldMixSTE(n_hyp=c["n_hyp"], **kw) if c["n_hyp"] > 0 else ManifoldMixSTE(**kw)
        T, K = c["T"], max(1, c["n_hyp"])
    model.load_state_dict(fixture_state(fx), strict=True)
    model.precision = "fp32"
    _MODELS[kind] = (model.cuda().eval(), T, K)
    return _MODELS[kind]


def sequences(lens, seed):
    """synthetic 2-D inputs (N, 17, 2) in [-1, 1] and 3-D targets (N, 17, 3), one pair of lists"""
    g = np.random.default_rng(seed)
    p2 = [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in lens]
    p3 = [(0.3 * g.standard_normal((n, 17, 3))).astype(np.float32) for n in lens]
    return p2, p3


def sequences_2d(T, seed=12):
    """three 2-D sequences around a model's window length: shorter than a window, whole windows, a last window that needs padding"""
    return sequences((T - 5, 2 * T, 2 * T + 5), seed)[0]


def to_numpy(ts):
    return [t.cpu().numpy() for t in ts]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}") if a.dtype.kind == "f" else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))
