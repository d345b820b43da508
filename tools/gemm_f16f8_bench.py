"""Micro-benchmark of the "f16f8" Linear forward (one fp16 + one block-scaled fp8 product per k-tile, mp_linear_fwd_f16f8) next to the shipped
split precision (three bf16 products, mp_linear_fwd_bf16x3) through the C ABI: the four Linear shapes of a MixSTE block, plain bias epilogue,
4 bytes of output per element in both (fp32 / planar bf16).  Operand planes hold random bytes of the right formats (timing only)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from manipose_amd import _lib
from gemm_bench import timeit

import argparse
import statistics

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("M", nargs="?", type=int, default=326349)
ap.add_argument("--tile", type=int, default=0, choices=[0, 128, 256], help='mp_set_option("gemm_tile"): 0 planner, 128 / 256 forced')
ap.add_argument("--m-list", default=None, help="comma-separated token counts: the crossover table of the f16f8 forward forms a block launches (qkv bias -> "
                "planar bf16, proj / fc2 residual -> fp32, fc1 GELU -> f16f8 planes), tile 128 against tile 256 alternating in this process, medians")
ap.add_argument("--form", default="f16f8", choices=["f16f8", "x3"], help="with --m-list: the operand form measured (x3: mp_linear_fwd_bf16x3, the same epilogues "
                "with planar bf16 outputs for qkv and fc1)")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream
M = args.M


def f16f8_operands(M, N, K):
    """random planes of the right formats (timing only)"""
    x = torch.randn(M, K, device="cuda")
    W = torch.randn(N, K, device="cuda") / K ** 0.5
    x16, W16 = x.half(), W.half()
    x8 = torch.cat([((x - x16.float()) * 2.0 ** 11).view(M, K // 4, 4), x16.float().view(M, K // 4, 4)], dim=2).to(torch.float8_e4m3fn).view(torch.uint8).reshape(M, 2 * K).contiguous()
    W8 = torch.cat([(W16.float() * 16).view(N, K // 4, 4), ((W - W16.float()) * 2.0 ** 15).view(N, K // 4, 4)], dim=2).to(torch.float8_e4m3fn).view(torch.uint8).reshape(N, 2 * K).contiguous()
    return x16, x8, W16, W8


def crossover(ms):
    """One line per (M, layer): median time of the 128 and the 256 tile (alternating, `reps` timings of 20 launches each), their ratio, the cost c of a
    128-tile relative to a quarter 256-tile that the pair implies under the planner's round model with this device's CU count, and the plan."""
    import ctypes as C
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = lambda t: t.data_ptr() if t is not None else None
    out4 = (C.c_int * 4)()
    print(f"# {args.form} forward forms, {cus} CUs, one queue, tiles alternating, median of {args.reps} x 20 launches; us per launch")
    print("# M layer N K epilogue t128_us t256_us t128/t256 rounds128 rounds256 implied_c plan_tile plan_persistent")
    for M in ms:
        for (N, K, name, epi, form) in [(1536, 512, "qkv", 0, 1), (512, 512, "proj", 2, 0), (2048, 512, "fc1", 1, 2), (512, 2048, "fc2", 2, 0)]:
            x16, x8, W16, W8 = f16f8_operands(M, N, K)
            b = torch.randn(N, device="cuda")
            r = torch.randn(M, N, device="cuda") if epi == 2 else None
            y = torch.empty(M, N, device="cuda", dtype=torch.float32 if form == 0 else torch.bfloat16)
            yl = torch.empty(M, N, device="cuda", dtype=torch.bfloat16) if form else None
            z = torch.empty(M, N, device="cuda", dtype=torch.bfloat16) if epi == 1 else None
            fn = lambda: lib.mp_linear_fwd_f16f8_ex(p(x16), p(x8), p(W16), p(W8), p(b), p(y), p(yl), p(z), p(r), None, None, None, None, 0, 1.0, 243, 17, M, N, K, epi, form, st)
            if args.form == "x3":             # planar bf16 hi / lo operands (random bf16 values: timing only)
                xh, xl, Wh, Wl = (torch.randn(sh, device="cuda").bfloat16() for sh in ((M, K), (M, K), (N, K), (N, K)))
                fn = lambda: lib.mp_linear_fwd_bf16x3(p(xh), p(xl), p(Wh), p(Wl), p(b), p(y), p(yl), p(z), p(r), M, N, K, epi, st)
            t = {128: [], 256: []}
            try:
                for _ in range(args.reps):
                    for tile in (128, 256):
                        _lib.check(lib.mp_set_option(b"gemm_tile", tile))
                        _lib.check(fn())
                        t[tile].append(timeit(fn) * 1e3)
            finally:
                _lib.check(lib.mp_set_option(b"gemm_tile", 0))
            t128, t256 = statistics.median(t[128]), statistics.median(t[256])
            r128 = -(-(-(-M // 128) * (N // 128)) // (2 * cus))
            r256 = -(-(-(-M // 256) * (N // 256)) // cus)
            _lib.check(lib.mp_gemm_plan(M, N, K, 8 if args.form == "f16f8" else 1, epi, 0, out4))
            print(f"{M} {name} {N} {K} {epi} {t128:.1f} {t256:.1f} {t128 / t256:.3f} {r128} {r256} {4.0 * r256 * t128 / (t256 * r128):.2f} {out4[0]} {out4[1]}", flush=True)


if args.m_list:
    crossover([int(v) for v in args.m_list.split(",")])
    sys.exit(0)
_lib.check(lib.mp_set_option(b"gemm_tile", args.tile))
tot = {"x3": 0.0, "f16f8": 0.0}
for (N, K, name) in [(1536, 512, "qkv"), (512, 512, "proj"), (1024, 512, "fc1"), (512, 1024, "fc2")]:
    x = torch.randn(M, K, device="cuda")
    W = torch.randn(N, K, device="cuda") / K ** 0.5
    xh, xl = torch.empty_like(x, dtype=torch.bfloat16), torch.empty_like(x, dtype=torch.bfloat16)
    Wh, Wl = torch.empty_like(W, dtype=torch.bfloat16), torch.empty_like(W, dtype=torch.bfloat16)
    lib.mp_split_bf16(x.data_ptr(), xh.data_ptr(), xl.data_ptr(), x.numel(), st)
    lib.mp_split_bf16(W.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), W.numel(), st)
    x16, W16 = x.half(), W.half()
    # correction planes: e4m3 bytes of random values of the real magnitudes (lo parts scaled as the format says)
    x8 = torch.cat([((x - x16.float()) * 2.0 ** 11).view(M, K // 4, 4), x16.float().view(M, K // 4, 4)], dim=2).to(torch.float8_e4m3fn).view(torch.uint8).reshape(M, 2 * K).contiguous()
    W8 = torch.cat([(W16.float() * 16).view(N, K // 4, 4), ((W - W16.float()) * 2.0 ** 15).view(N, K // 4, 4)], dim=2).to(torch.float8_e4m3fn).view(torch.uint8).reshape(N, 2 * K).contiguous()
    del x
    b = torch.randn(N, device="cuda")
    yh, yl = torch.empty(M, N, device="cuda", dtype=torch.bfloat16), torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    y32 = torch.empty(M, N, device="cuda")
    p = lambda t: t.data_ptr() if t is not None else None
    t3 = timeit(lambda: lib.mp_linear_fwd_bf16x3(p(xh), p(xl), p(Wh), p(Wl), p(b), p(yh), p(yl), None, None, M, N, K, 0, st))
    t8 = timeit(lambda: lib.mp_linear_fwd_f16f8(p(x16), p(x8), p(W16), p(W8), p(b), p(y32), M, N, K, st))
    tot["x3"] += t3; tot["f16f8"] += t8
    fl = 2.0 * M * N * K
    print(f"{name:5s} M={M} N={N} K={K}: x3 {t3 * 1e3:7.1f} us {fl / t3 / 1e9:6.1f} TF algorithmic | f16f8 {t8 * 1e3:7.1f} us {fl / t8 / 1e9:6.1f} TF algorithmic  (x{t3 / t8:.2f})", flush=True)
print(f"block total: x3 {tot['x3'] * 1e3:.0f} us, f16f8 {tot['f16f8'] * 1e3:.0f} us; x16 blocks = {tot['x3'] * 16:.1f} / {tot['f16f8'] * 16:.1f} ms")
