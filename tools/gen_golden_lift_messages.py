"""Generates tests/golden/lift_messages.json: the exception type and the complete message of every bad call in the table of
tests/test_lift_messages_host.py (its CASES and provoke(): the recording and the test run the same code).  Host only, no GPU, no library.

    python tools/gen_golden_lift_messages.py [out.json]

Then lists the raise statements of the lifting bindings (manipose_amd/lift_args.py, lift_ops.py, lift_views.py, lifting.py - whichever exist - and
the lift_*_options functions of hpe/_entry.py) that no row of the table ended in, so that the rows left out can be named line by line.

The committed file was run against d828fa9 ("Lifting kernels: one geometry header for rotation, camera model, solves"), the last commit at
which manipose_amd/lifting.py held all the bindings and their argument checks; it is not to be re-recorded to make a changed message pass."""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hpe"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_lift_messages_host as table  # noqa: E402


def raise_sites():
    """{(path, first line, last line): function name} of the raise statements the table is to reach"""
    sites = {}
    paths = [os.path.join(ROOT, "manipose_amd", n + ".py") for n in ("lift_args", "lift_ops", "lift_views", "lifting")]
    for path in [p for p in paths if os.path.exists(p)] + [os.path.join(ROOT, "hpe", "_entry.py")]:
        for fn in ast.walk(ast.parse(open(path).read())):
            if isinstance(fn, ast.FunctionDef) and (not path.endswith("_entry.py") or (fn.name.startswith("lift_") and fn.name.endswith("_options"))):
                sites.update({(path, n.lineno, n.end_lineno): fn.name for n in ast.walk(fn) if isinstance(n, ast.Raise)})
    return sites


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else table.GOLD
    out, hit = {}, set()
    for name in table.CASES:
        kind, message, e = table.provoke(name)
        out[name] = {"type": kind, "message": message}
        tb = e.__traceback__
        while tb.tb_next is not None:
            tb = tb.tb_next
        hit.add((tb.tb_frame.f_code.co_filename, tb.tb_lineno))
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    sites = raise_sites()
    src = {}
    for (p, line, last), fn in sorted(sites.items()):
        if not any((p, l) in hit for l in range(line, last + 1)):
            text = src.setdefault(p, open(p).read().splitlines())[line - 1].strip()
            print(f"not reached: {os.path.relpath(p, ROOT)}:{line} {fn}: {text[:110]}")
    print(f"lift_messages: ok {len(out)} rows, {len(sites)} raise statements, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
