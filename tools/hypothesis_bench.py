"""Times mp_hypothesis_stats at the evaluation shape (train.batch_size_test 10 x K 5 x T 243 windows, and the 20 of a flip-doubled batch)
with HIP events, and beside it the same quantities composed from torch device ops - the yardstick a user would write today, not code
under test.  Algorithmic bytes per frame: (K 51 + K + 51) floats read once.
    python tools/hypothesis_bench.py [--reps 200] [--rounds 5]
Prints per shape: median and min..max over the rounds of the mean time per call, and the achieved GB/s of the kernel."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_composition(p, s, g, scale):
    """Every quantity of the two rows from torch ops (sums on the device, no host sync inside)."""
    B, K, T = p.shape[:3]
    q, y = scale * p, scale * g
    e = (q - y[:, None]).norm(dim=-1)                                  # (B, K, T, 17)
    E = e.sum(-1)                                                      # (B, K, T)
    ko, ks = E.argmin(1), s.argmax(1)
    order = torch.argsort(s, dim=1, descending=True, stable=True)
    rank = torch.argsort(order, dim=1, stable=True)
    topm = torch.cummin(E.gather(1, order), dim=1).values
    ej, kj = e.min(1)
    w = (s[..., None, None] * q).sum(1)
    spread = (s[..., None] * (q - w[:, None]).pow(2).sum(-1)).sum(1).sqrt()
    iu = torch.triu_indices(K, K, 1, device=p.device)
    pair = (q[:, iu[0]] - q[:, iu[1]]).norm(dim=-1).sum((1, 3)) * (2.0 / max(K * (K - 1), 1))
    floats = torch.cat([torch.stack([E.gather(1, ks[:, None]).sum(), E.gather(1, ko[:, None]).sum(), ej.sum(), (w - y).norm(dim=-1).sum(),
                                     s.gather(1, ko[:, None]).sum(), s.gather(1, ks[:, None]).sum(), pair.sum()]),
                        topm.sum((0, 2)), ej.sum((0, 1)), spread.sum((0, 1)), s.sum((0, 2))])
    counts = torch.cat([(ko == ks).sum()[None], torch.bincount(rank.gather(1, ko[:, None]).reshape(-1), minlength=K),
                        torch.bincount(ko.reshape(-1), minlength=K), torch.bincount(ks.reshape(-1), minlength=K),
                        torch.bincount(kj.reshape(-1), minlength=K)])
    return floats, counts


def timed(fn, reps, rounds):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)                     # us per call
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hypothesis_bench: needs an MI355X; nothing is measured without one")
    from manipose_amd import _lib
    lib = _lib.load()
    for B, K, T in ((10, 5, 243), (20, 5, 243)):
        g = torch.Generator(device="cuda").manual_seed(B)
        y = 0.3 * torch.randn(B, T, 17, 3, device="cuda", generator=g)
        p = y[:, None] + 0.03 * torch.randn(B, K, T, 17, 3, device="cuda", generator=g)
        s = torch.softmax(torch.randn(B, K, T, device="cuda", generator=g), dim=1)
        sums = torch.empty(int(lib.mp_hypothesis_stats_row_floats()), device="cuda")
        counts = torch.empty(int(lib.mp_hypothesis_stats_row_counts()), dtype=torch.int64, device="cuda")
        scratch = torch.empty(int(lib.mp_hypothesis_stats_scratch_floats(B * T)), device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def kernel():
            _lib.check(lib.mp_hypothesis_stats(p.data_ptr(), s.data_ptr(), y.data_ptr(), B, K, T, 1000.0, 1000.0, sums.data_ptr(), counts.data_ptr(),
                                               None, None, scratch.data_ptr(), scratch.numel(), st), "mp_hypothesis_stats")

        kernel()
        f, c = torch_composition(p, s, y, 1000.0)
        torch.cuda.synchronize()
        fi = torch.tensor(list(range(1, 8)) + list(range(8, 8 + K)) + list(range(16, 50)) + list(range(50, 50 + K)), device="cuda")
        ci = torch.tensor([0] + [o + k for o in (1, 9, 17, 25) for k in range(K)], device="cuda")
        rel = ((f - sums[fi]).abs() / sums[fi].abs().clamp_min(1e-30)).max().item()
        print(f"B={B}: kernel against the composition (float32 both, random data without planted gaps): largest relative difference of a sum "
              f"{rel:.2e}, counts differ in {(c != counts[ci]).sum().item()} of {ci.numel()} slots", flush=True)
        k = timed(kernel, a.reps, a.rounds)
        t = timed(lambda: torch_composition(p, s, y, 1000.0), max(a.reps // 10, 5), a.rounds)
        nbytes = B * T * (K * 51 + K + 51) * 4
        print(f"B={B} K={K} T={T}: mp_hypothesis_stats {k[0]:.1f} us per call (min {k[1]:.1f}, max {k[2]:.1f}; two launches), "
              f"{nbytes / k[0] / 1e3:.1f} GB/s of {nbytes / 1e6:.2f} MB; torch composition {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f}); "
              f"ratio {t[0] / k[0]:.1f}", flush=True)


if __name__ == "__main__":
    main()
