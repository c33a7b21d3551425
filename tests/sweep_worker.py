"""python -m tests.sweep_worker OP 'RECORD' ['RECORD' ...] -- the cases of tests/sweep.py given as records, through
tests/test_gpu_sweep.run_cases in this process; the last line is WORKER_MARK and the repr of [(case, what differs)].
The library reads G1S_K3 once per process, so tests/test_gpu_sweep.py starts this with G1S_K3=stream for the diff cases that
ask for the stream chain (as tests/test_gpu_selfcheck.py starts tests/k3_mode_digest.py)."""
import ast
import sys

from tests import test_gpu_sweep as T


def main(argv) -> int:
    op, cases = argv[0], [ast.literal_eval(r) for r in argv[1:]]
    fails = T.run_cases(op, cases)
    print(T.WORKER_MARK + repr(fails), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
