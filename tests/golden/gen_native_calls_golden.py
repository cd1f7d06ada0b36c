#!/usr/bin/env python3
"""Generate tests/golden/native_calls.json: the native calls the Python glue makes on the cases of tests/native_call_cases.py, recorded under the CPU emulation library.

The fixture states what a refactor of the Python layer must leave unchanged, so it is written ONCE, on a checkout of the commit BEFORE the change it is to hold, and
never regenerated from the code under test: copy this script and tests/native_call_cases.py into that checkout and run

    python tests/golden/gen_native_calls_golden.py <commit the checkout is at>

The commit is stored in the fixture.  The whole-model step is stored as the SHA-256 of its canonical trace plus the call count per entry; the other cases in full.

One stated exception: an entry RETIRED after that commit is written as the call of the entry that replaced it (`RETIRED` below, argument for argument), in the cases
only — the whole-model step never called one.  The stand-alone Ghost blocks went from the first depthwise 3x3 entries to the `ach_train_dwconv` family the model runs."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, 'tests'), REPO]

import native_call_cases as NC                                             # noqa: E402


RETIRED = {  # [name, x, w, y, B, C, H, W, flip, s] -> dwconv(x, w, no bias, y, B, C, H, W, k = 3, flip, s);  [name, x, dz, dw, B, C, H, W, s] -> dwconv_wgrad(..., k = 3, s)
    'ach_train_dw3x3': lambda c: ['ach_train_dwconv', c[1], c[2], 0, c[3]] + c[4:8] + [3, c[8], c[9]],
    'ach_train_dw3x3_wgrad': lambda c: ['ach_train_dwconv_wgrad'] + c[1:8] + [3, c[8]],
}


def main(commit):
    cases = {name: [RETIRED.get(c[0], list)(c) for c in NC.record(fn)] for name, fn in NC.CASES.items()}
    step = NC.record(NC.train_step)
    assert not set(NC.counts(step)) & set(RETIRED)
    assert NC.digest(NC.record(NC.train_step)) == NC.digest(step), 'the whole-model step does not make the same calls twice'
    out = {'commit': commit, 'cases': cases, 'train_step': {'calls': len(step), 'counts': NC.counts(step), 'sha256': NC.digest(step)}}
    path = os.path.join(HERE, 'native_calls.json')
    with open(path, 'w') as f:
        f.write('{\n "commit": %s,\n "cases": {\n' % json.dumps(commit))
        f.write(',\n'.join('  %s: [\n%s\n  ]' % (json.dumps(n), ',\n'.join('   ' + NC.canonical(c) for c in t)) for n, t in cases.items()))
        f.write('\n },\n "train_step": %s\n}\n' % json.dumps(out['train_step'], indent=1).replace('\n', '\n '))
    assert json.load(open(path)) == out
    print(path, {n: len(t) for n, t in cases.items()}, out['train_step']['calls'])


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
