#!/usr/bin/env python3
"""Generate tests/golden/ln_gemm_parent.json / .npz: what the LayerNorm-prologue GEMMs of the 16-bit engines (the patchify convs and the LayerNorm + qkv projections)
and everything behind them computed BEFORE k_lngemm.h, on the CPU emulation library — the cases of tests/ln_gemm_cases.py, every tensor as the SHA-256 of its bits and
the small ones whole.

The fixture states what a change of these kernels must leave unchanged bit for bit, so it is written on a checkout of the commit before such a change and never
regenerated from the code under test.  Copy this script and tests/ln_gemm_cases.py into that checkout and run

    python tests/golden/gen_ln_gemm_parent.py <commit the checkout is at>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, 'tests'), REPO]

import ln_gemm_cases as LC                                                  # noqa: E402
from emu_util import emu_library                                           # noqa: E402


def main(commit):
    digests, full = {}, {}
    for name, res, batch in LC.CASES:
        for storage in LC.STORAGE:
            cid = LC.case_id(name, res, batch, storage)
            got, _ = LC.run(emu_library(), name, res, batch, storage)
            digests[cid] = {k: LC.digest(b) for k, b in got.items()}
            for k, b in got.items():
                if b.numel() <= LC.FULL_ELEMS:
                    full[cid + '::' + k] = b.numpy()
            print(cid, {k: tuple(b.shape) for k, b in got.items()})
    with open(LC.FIXTURE_JSON, 'w') as f:
        json.dump({'commit': commit, 'sha256': digests}, f, indent=1)
        f.write('\n')
    np.savez_compressed(LC.FIXTURE_NPZ, **full)
    print(LC.FIXTURE_JSON, os.path.getsize(LC.FIXTURE_JSON), 'bytes;', LC.FIXTURE_NPZ, os.path.getsize(LC.FIXTURE_NPZ), 'bytes,', len(full), 'tensors whole')


if __name__ == '__main__':
    main(sys.argv[1])
