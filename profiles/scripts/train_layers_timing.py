"""Forward + backward time of the stand-alone Ghost blocks (achelous_amd/train_ops.py) on the GPU, this tree against another BUILT checkout of the project (the parent
commit: its stand-alone blocks ran the first depthwise 3x3 entries, this tree's run the `ach_train_dwconv` family the model runs).  The two large cases of
tests/test_train_ops.py.  One child process per leg (two trees cannot share a process: one package name), legs alternated other / this / other / this; per leg and case
10 warm-up calls, then 50 calls each between device events behind a synchronise, the median reported with min .. max.
usage: python profiles/scripts/train_layers_timing.py --other PATH_TO_BUILT_CHECKOUT [--out profiles/train_layers_timing.txt]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
CASES = [('GhostBottleneck(192, 192, 96)', 'GhostBottleneck', (192, 192, 96), (64, 192, 20, 20)), ('GhostModule(32, 9)', 'GhostModule', (32, 9), (8, 32, 320, 320))]
WARMUP, CALLS = 10, 50


def leg(tree):
    sys.path.insert(0, tree)
    import torch
    from achelous_amd import train_ops
    out = {}
    for name, cls, args, shape in CASES:
        torch.manual_seed(0)
        m = getattr(train_ops, cls)(*args).cuda().train()
        x = torch.randn(*shape).cuda().requires_grad_(True)
        dy = torch.randn_like(m(x))
        ms = []
        for k in range(WARMUP + CALLS):
            for p in (x, *m.parameters()):
                p.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            m(x).backward(dy)
            e1.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        out[name] = (ms[len(ms) // 2], ms[0], ms[-1])
    print('LEG ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other', help='root of the other built checkout')
    ap.add_argument('--out')
    ap.add_argument('--leg', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg)
    if not a.other:
        ap.error('--other is required')
    trees = [('other', os.path.abspath(a.other)), ('this', REPO)] * 2
    runs = []
    for label, tree in trees:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', tree], check=True, capture_output=True, text=True, timeout=600)
        runs.append((label, json.loads([l for l in r.stdout.splitlines() if l.startswith('LEG ')][-1][4:])))
    lines = [f'stand-alone Ghost blocks, forward + backward, fp32, ms per call: median of {CALLS} after {WARMUP} warm-up calls (min .. max); legs in the order run',
             'other = the checkout given by --other (the parent commit: ach_train_dw3x3 / _wgrad), this = this tree (ach_train_dwconv / _wgrad)']
    ok = True
    for name, _, _, shape in CASES:
        lines.append(f'  {name} on {shape}')
        for label, res in runs:
            med, lo, hi = res[name]
            lines.append(f'    {label:5s} {med:8.3f}  ({lo:.3f} .. {hi:.3f})')
        slowest_other = max(res[name][0] for label, res in runs if label == 'other')
        mine = [res[name][0] for label, res in runs if label == 'this']
        good = all(t <= slowest_other for t in mine)
        ok = ok and good
        lines.append(f'    this {"<=" if good else ">"} the slower of the other\'s two runs ({slowest_other:.3f}): {", ".join(f"{t:.3f}" for t in mine)}')
    lines.append('verdict: ' + ('no stand-alone block is slower on the model\'s depthwise kernels' if ok else 'SLOWER than the other tree'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
