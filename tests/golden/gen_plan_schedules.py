#!/usr/bin/env python3
"""Generate tests/golden/plan_schedules.json: streams, joins and cross-forward marks of the plan set of tests/plan_schedules.py, built on the CPU emulation library.

The fixture states what a change of the host-side scheduling code must leave unchanged, so it is written on a checkout of the commit BEFORE such a change (with
ach_op_sync added, if that checkout lacks it) and never regenerated from the code under test, unless the change of schedule is the point of the commit — then the
diff of the fixture is the review.  Copy this script and tests/plan_schedules.py into that checkout and run

    python tests/golden/gen_plan_schedules.py <commit the checkout is at> [directory for the full listings]

With a directory, every launch of every plan (name, stream, four masks, in plan order) is also written there, one file per plan, for a one-time A/B of two trees."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, 'tests'), REPO]

import plan_schedules as PS                                                # noqa: E402
from emu_util import emu_library                                           # noqa: E402


def main(commit, full_dir=None):
    plans = {}
    for pid, full in PS.all_plans(emu_library()):
        plans[pid] = PS.summary(full)
        if full_dir:
            os.makedirs(full_dir, exist_ok=True)
            with open(os.path.join(full_dir, pid.replace('/', '__') + '.json'), 'w') as f:
                f.write(json.dumps(full, indent=0) if isinstance(full, dict) else '[\n' + ',\n'.join(json.dumps(o) for o in full) + '\n]\n')
    with open(PS.SCHEDULES_JSON, 'w') as f:
        f.write('{\n "commit": %s,\n "plans": {\n' % json.dumps(commit))
        f.write(',\n'.join('  %s: %s' % (json.dumps(pid), PS.canonical(p)) for pid, p in plans.items()))
        f.write('\n }\n}\n')
    print(PS.SCHEDULES_JSON, os.path.getsize(PS.SCHEDULES_JSON), 'bytes,', len(plans), 'plans,', sum('error' in p for p in plans.values()), 'of them failures')


if __name__ == '__main__':
    main(*sys.argv[1:3])
