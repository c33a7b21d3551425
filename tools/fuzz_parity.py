#!/usr/bin/env python3
"""tools/fuzz_parity.py OP [N] [SEED] -- N cases of tests/sweep.py's edge-weighted generator for one operation (diff, render,
denoise, denoise_t, estimate, resize) through the comparison of tests/test_gpu_sweep.py: the device against the operation's
reference, bit for bit.  The suite runs the same generator at its committed (seed, n); a long hand run differs in N and SEED
only.  Every failing case is printed as `FAIL RECORD :: what differs`.

  tools/fuzz_parity.py OP --case 'RECORD' [--case 'RECORD' ...]   replays pasted records

A diff case that asks for the stream chain (k3 = "stream") runs in a child (tests/sweep_worker.py) started with G1S_K3=stream, which the
library reads once per process; started with G1S_K3=stream itself, the tool runs such cases in place.
Exit status: 0 when every case agrees, 1 otherwise."""
import argparse
import ast
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import sweep as S  # noqa: E402

CHUNK = 16  # cases per call of run_cases: objects are reused inside a call, as inside a chunk of the suite


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("op", choices=S.OPS)
    ap.add_argument("n", nargs="?", type=int, default=100)
    ap.add_argument("seed", nargs="?", type=int, default=1)
    ap.add_argument("--case", action="append", default=[], help="a case record as a failure message prints it")
    a = ap.parse_args(argv)
    from tests import test_gpu_sweep as T

    todo = [ast.literal_eval(r) for r in a.case] if a.case else S.cases(a.op, a.seed, a.n)
    for c in todo:
        if c.get("op") != a.op:
            ap.error(f"a record of {c.get('op')!r} given to {a.op!r}")
    if not a.case:
        print(f"{a.op}: seed {a.seed}, list sha256 {S.digest(todo)}", flush=True)
    t0 = time.time()
    bad = set()
    for k in range(0, len(todo), CHUNK):
        fails = T.run_cases(a.op, todo[k:k + CHUNK])
        if fails:
            print(T.report(fails), flush=True)
        bad |= {repr(c) for c, _ in fails}
    print(f"{len(todo)} cases, {len(bad)} failures, {time.time() - t0:.0f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
