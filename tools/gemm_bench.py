"""Micro-benchmark of the bf16 GEMM kernels through the C ABI (one MI355X): TFLOP/s per shape and variant."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from manipose_amd import _lib

lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def crossover(ms, reps):
    """The plain bf16 dgrads (dx = dy W, and the gelu'-multiplying one of fc1) of a block, tile 128 against tile 256 of the tiled template, alternating
    in this process, medians; same columns as tools/gemm_f16f8_bench.py --m-list.  (Shapes the persistent kernel serves show the same time twice.)"""
    import ctypes as C
    import statistics
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out4 = (C.c_int * 4)()
    print(f"# bf16 dgrad forms, {cus} CUs, one queue, tiles alternating, median of {reps} x 20 launches; us per launch")
    print("# M layer N K epilogue t128_us t256_us t128/t256 rounds128 rounds256 implied_c plan_tile plan_persistent")
    for M in ms:
        # dgrad of a Linear(K_in -> N_out): dx[M, K_in] = dy[M, N_out] W[N_out, K_in]; the GEMM's (N, K) are (K_in, N_out)
        for (N_out, K_in, name, dgelu) in [(1536, 512, "qkv", 0), (512, 512, "proj", 0), (2048, 512, "fc1", 0), (512, 2048, "fc2", 1)]:
            dy = torch.randn(M, N_out, device="cuda").bfloat16()
            W = (torch.randn(N_out, K_in, device="cuda") / K_in ** 0.5).bfloat16()
            dx = torch.empty(M, K_in, device="cuda", dtype=torch.bfloat16)
            z = torch.rand(M, K_in, device="cuda").bfloat16() if dgelu else None
            fn = lambda: lib.mp_linear_bwd_f16(dy.data_ptr(), None, W.data_ptr(), dx.data_ptr(), z.data_ptr() if dgelu else None, None, None, None, None,
                                               M, N_out, K_in, 0, 0, None, None, 0, st)
            t = {128: [], 256: []}
            try:
                for _ in range(reps):
                    for tile in (128, 256):
                        _lib.check(lib.mp_set_option(b"gemm_tile", tile))
                        _lib.check(fn())
                        t[tile].append(timeit(fn) * 1e3)
            finally:
                _lib.check(lib.mp_set_option(b"gemm_tile", 0))
            t128, t256 = statistics.median(t[128]), statistics.median(t[256])
            r128 = -(-(-(-M // 128) * (K_in // 128)) // (2 * cus))
            r256 = -(-(-(-M // 256) * (K_in // 256)) // cus)
            _lib.check(lib.mp_gemm_plan(M, K_in, N_out, 0, 3 if dgelu else 0, 0, out4))
            print(f"{M} {name}.dgrad {K_in} {N_out} {3 if dgelu else 0} {t128:.1f} {t256:.1f} {t128 / t256:.3f} {r128} {r256} {4.0 * r256 * t128 / (t256 * r128):.2f} {out4[0]} {out4[1]}", flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("M", nargs="?", type=int, default=66096)
    ap.add_argument("--tile", type=int, default=0, choices=[0, 128, 256], help='mp_set_option("gemm_tile"): 0 planner, 128 / 256 forced')
    ap.add_argument("--m-list", default=None, help="comma-separated token counts: crossover table of the bf16 dgrads, tile 128 against 256")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.m_list:
        crossover([int(v) for v in args.m_list.split(",")], args.reps)
        return
    _lib.check(lib.mp_set_option(b"gemm_tile", args.tile))
    M = args.M
    for (N, K, name) in [(1536, 512, "qkv"), (512, 512, "proj"), (1024, 512, "fc1"), (512, 1024, "fc2")]:
        x = torch.randn(M, K, device="cuda").bfloat16()
        W = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
        b = torch.randn(N, device="cuda")
        r = torch.randn(M, N, device="cuda")
        dy = torch.randn(M, N, device="cuda").bfloat16()
        dy32 = dy.float()
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        y32 = torch.empty(M, N, device="cuda")
        z = torch.empty_like(y)
        dx = torch.empty(M, K, device="cuda")
        dW, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        slab = torch.empty(int(lib.mp_linear_bwd_slab_floats(N, K)), device="cuda")
        fl = 2.0 * M * N * K
        res = {}
        res["fwd_bias"] = timeit(lambda: lib.mp_linear_fwd_bf16(x.data_ptr(), W.data_ptr(), b.data_ptr(), y.data_ptr(), None, None, M, N, K, 0, st))
        res["fwd_gelu"] = timeit(lambda: lib.mp_linear_fwd_bf16(x.data_ptr(), W.data_ptr(), b.data_ptr(), y.data_ptr(), z.data_ptr(), None, M, N, K, 1, st))
        res["fwd_resid"] = timeit(lambda: lib.mp_linear_fwd_bf16(x.data_ptr(), W.data_ptr(), b.data_ptr(), y32.data_ptr(), None, r.data_ptr(), M, N, K, 2, st))
        res["bwd_bf16dy(dgrad+wgrad)"] = timeit(lambda: lib.mp_linear_bwd_bf16(dy.data_ptr(), 0, x.data_ptr(), W.data_ptr(), dx.data_ptr(), 1, dW.data_ptr(), db.data_ptr(), M, N, K, slab.data_ptr(), slab.numel(), st)) / 2
        res["bwd_f32dy(dgrad+wgrad)"] = timeit(lambda: lib.mp_linear_bwd_bf16(dy32.data_ptr(), 1, x.data_ptr(), W.data_ptr(), dx.data_ptr(), 1, dW.data_ptr(), db.data_ptr(), M, N, K, slab.data_ptr(), slab.numel(), st)) / 2
        print(f"{name:5s} M={M} N={N} K={K}: " + "  ".join(f"{k}={fl / (v * 1e-3) / 1e12:6.1f}TF" for k, v in res.items()), flush=True)


if __name__ == "__main__":
    main()
