"""GPU box: parity of the streaming gradient kernel (DIRT_FLAG_GRAD_STREAM) against the CPU oracle on frames whose sides are
multiples of 32 -- random sizes, meshes (split / shared / hostile / tiny), both quirk-Q1 modes, batches, with and without the
forward's state -- at the tight tolerance: the `stream` mode of tests/fuzz_parity.py (a fixed-seed slice of it runs under
pytest: tests/test_gpu_grad_stream.py), open-ended.
usage: python tools/check_stream.py [seconds] [seed]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import fuzz_parity  # noqa: E402


def run(budget, seed):
    fails = []
    n = fuzz_parity.run(budget=budget, seed=seed, stream=True, failures=fails)
    return n, fails


if __name__ == '__main__':
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.
    n, fails = run(budget, int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    for f in fails[:20]:
        print('MISMATCH', f)
    print('check_stream: %d cases, %d mismatches' % (n, len(fails)))
    sys.exit(1 if fails else 0)
