"""Generates tests/golden/attn_bits.json: the SHA-256 and the shape of every output tensor of the ten public attention entry points on the
rows of tests/test_gpu_attention_kernels.py (its bits_table() / bits_digests(): the recording and the test run the same code).  Digests only;
the inputs are regenerated from their seeds.  Needs an MI355X.

    MANIPOSE_HIP_LIB=<library built at the commit to record> python tools/gen_golden_attn_bits.py [out.json]

Runs the table twice: a tensor whose digest does not repeat is named and left out of the file (the attention kernels use no atomics: none did).

The committed file was run against f55a777 ("Lifting bindings: one set of argument checks, three modules by layer"), the last commit at which
the attention launchers read their softmax scale and gradient form from thread-local overrides; it is not to be re-recorded to make a changed
kernel pass."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_attention_kernels as bits  # noqa: E402


def main():
    from manipose_amd import _lib
    path = sys.argv[1] if len(sys.argv) > 1 else bits.GOLD_BITS
    lib = _lib.load()
    first, second = bits.bits_digests(lib), bits.bits_digests(lib)
    unstable = sorted(k for k in first if first[k] != second[k])
    for k in unstable:
        print("does not repeat, left out:", k)
    assert not [k for k in unstable if "_fwd" in k], "a forward output does not repeat"
    out = {k: v for k, v in first.items() if k not in unstable}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}" for k in sorted(out)) + "\n}\n")      # a tensor a line
    print("attn_bits: ok", _lib.LIB_PATH, len(bits.bits_table()), "rows", len(out), "tensors", len(unstable), "unstable", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
