"""The table behind profiles/train_primitive_parity.txt: every case of tests/test_train_functional.py (the named cases and the replay of a live training step) run
WITHOUT asserting, one line per compared tensor: native error and torch-float32 error (the yardstick) against the float64 truth, their ratio, the bound of the test.

    python profiles/scripts/train_primitive_parity.py cpu  [replay batch]     the kernels under the emulation library
    python profiles/scripts/train_primitive_parity.py cuda [replay batch]     the HIP kernels

The last lines give the largest ratio among tensors whose yardstick is above the floor: F_YARD of the test is twice that, rounded up (at most 16)."""
import contextlib
import io
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import test_train_functional as T          # noqa: E402
from achelous_amd import train_ops         # noqa: E402


def main():
    dev = sys.argv[1] if len(sys.argv) > 1 else 'cpu'
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else (2 if dev == 'cpu' else 8)
    if dev == 'cpu':
        from emu_util import emu_library
        train_ops._lib.test_library = emu_library()
    T.PARITY_LOG = log = []
    problems, said = [], io.StringIO()            # what the cases print (the share each stated condition left out) goes under the table
    for name, case in T._cases(dev):
        n0, t0 = len(log), time.time()
        try:
            with contextlib.redirect_stdout(said):
                case()
        except AssertionError as e:                     # a stated condition (ReLU mask, excluded share) that did not hold: reported, never hidden
            problems.append(f'{name}: {e}')
        log[n0:] = [(w or name, *rest) for w, *rest in log[n0:]]
        print(f'# {name}: {time.time() - t0:.1f} s', file=sys.stderr, flush=True)
    n_named = len(log)
    t0 = time.time()
    try:
        with contextlib.redirect_stdout(said):
            T._replay(dev, batch)
    except AssertionError as e:
        problems.append(f'replay: {e}')
    print(f'# replay: {time.time() - t0:.1f} s', file=sys.stderr, flush=True)
    print(f'device {dev}; F_YARD = {T.F_YARD}; floor 2^-20 = {T.FLOOR:.2e}; bound = min(tolerance, max(floor, F_YARD x yardstick)); replay batch {batch}')
    print(f'{"case":110s} {"tensor":22s} {"native":>9s} {"yardstick":>9s} {"ratio":>6s} {"bound":>9s}')
    worst = (0.0, None)
    for i, (what, tensor, err, yard, bound) in enumerate(log):
        if i == n_named:
            print('--- replay of a live training step')
        ratio = err / yard if yard > 0 else math.inf if err > 0 else 0.0
        if yard > T.FLOOR and ratio > worst[0]:
            worst = (ratio, f'{what}: {tensor}')
        print(f'{what[:110]:110s} {tensor:22s} {err:9.2e} {yard:9.2e} {ratio:6.2f} {bound:9.2e}{"" if err < bound else "   OUT OF BOUND"}')
    print(f'{len(log)} tensors; largest native / yardstick ratio among tensors with a yardstick above the floor: {worst[0]:.2f} ({worst[1]})')
    print(f'largest native error among tensors with a yardstick at or below the floor: {max((e for _, _, e, y, _ in log if y <= T.FLOOR), default=0.0):.2e} (floor {T.FLOOR:.2e})')
    print('--- stated conditions')
    print(said.getvalue(), end='')
    for p in problems:
        print('CONDITION NOT MET:', p)


if __name__ == '__main__':
    main()
