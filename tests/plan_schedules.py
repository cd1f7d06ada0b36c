"""The plan set behind tests/golden/plan_schedules.json: which stream every launch runs on and which launches carry a join or cross-forward mark, for the
option sets that change the schedule (csrc/engine_schedule.h).  Shared by the generator (tests/golden/gen_plan_schedules.py) and the test that rebuilds every plan
on the CPU emulation library (tests/test_abi_and_host.py)."""
import json
import os

import torch

from achelous_amd.engine import DTYPE_F16, DTYPE_F32, NativeEngine
from achelous_amd.synth import condition_state_dict
from golden_util import GOLDEN_DIR

SCHEDULES_JSON = os.path.join(GOLDEN_DIR, 'plan_schedules.json')
CONFIGS = ('en_s0', 'mv_s2', 'en_s0_cdf', 'en_s0_pn2')
# the option sets that change the schedule; radar_start = 4 is the EdgeNeXt plan that must fail (no stage records the radar release)
OPTION_SETS = ([{}, {'streams': 0}, {'pipeline': 1}] + [{'pipeline': 1, 'dec_fork': v} for v in (0, 2, 3)] + [{'head_stream': 1}] +
               [{'split_decoders': v} for v in (1, 2)] + [{'pipeline': 1, 'head_stream': 1}, {'pipeline': 1, 'split_decoders': 1}] +
               [{'point_stream2': v} for v in (0, 1, 3)] + [{'radar_start': v} for v in (-1, 0, 1, 2, 3, 4)])


def option_id(opts):
    return ','.join(f'{k}={v}' for k, v in opts.items()) or 'plain'


def engines_of(config):
    """[(tag, dtype, resolution)]: fp32 at 64 x 64, fp16 storage at 96 x 96 (128 x 128 for mv_s2)"""
    return [('f32', DTYPE_F32, 64), ('f16', DTYPE_F16, 128 if config == 'mv_s2' else 96)]


def setup(config):
    """(constructor keywords without the resolution, state dict, points per frame)"""
    if config == 'en_s0_pn2':     # no fixture of its own: the drop-in module's parameter tree, as test_emulated_other_widths_match_oracle builds one
        from achelous_amd.nets import Achelous
        kw = dict(num_det=7, num_seg=9, phi='S0', backbone='en', neck='gdf', pc_seg='pn2', pc_channels=5, pc_classes=8, nano_head=True, spp=True)
        return kw, condition_state_dict({k: torch.zeros_like(v) for k, v in Achelous(resolution=64, **kw).state_dict().items()}, seed=0), 512
    with open(os.path.join(GOLDEN_DIR, config + '.keys.json')) as f:
        meta = json.load(f)
    kw = {k: v for k, v in meta['ctor'].items() if k != 'resolution'}
    return kw, condition_state_dict({k: torch.zeros(s, dtype=getattr(torch, dt)) for k, s, dt in meta['keys']}, seed=0), 48


def listing(lib, kw, sd, npts, dtype, res, opts):
    """every launch of one plan: [name, stream, wait, signal, xwait, xsignal] in plan order, or {'error': text} for a plan that fails"""
    eng = NativeEngine(lib, num_det=kw['num_det'], num_seg=kw['num_seg'], phi=kw['phi'], backbone=kw['backbone'], resolution=res, pc_channels=kw['pc_channels'],
                       pc_classes=kw['pc_classes'], num_points=npts, nano_head=kw['nano_head'], spp=kw['spp'], dtype=dtype, neck=kw.get('neck', 'gdf'),
                       pc_seg=kw.get('pc_seg', 'pn'))
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.load_state_dict(sd)
    try:
        eng.plan(1)
        return [[o['op'], o['stream'], o['wait'], o['signal'], o['xwait'], o['xsignal']] for o in eng.op_schedule()]
    except Exception as e:
        return {'error': f'{type(e).__name__}: {e}'}
    finally:
        eng.destroy()


def summary(full):
    """what the committed file keeps of one listing: launches per stream with the first and last name, and every launch that has a mask set as
    [name, stream, index within the stream, wait, signal, xwait, xsignal]"""
    if isinstance(full, dict):
        return full
    streams, marked = {}, []
    for name, stream, *masks in full:
        s = streams.setdefault(str(stream), {'n': 0, 'first': name})
        if any(masks):
            marked.append([name, stream, s['n']] + masks)
        s['n'] += 1
        s['last'] = name
    return {'streams': streams, 'marked': marked}


def canonical(plan):
    """the file's text of one summary: one line per stream and per marked launch, so that a change of schedule reads as a diff of lines"""
    if 'error' in plan:
        return json.dumps(plan)
    streams = ',\n'.join('    %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in plan['streams'].items())
    marked = ',\n'.join('    ' + json.dumps(m) for m in plan['marked'])
    return '{\n   "streams": {\n%s},\n   "marked": [\n%s]}' % (streams, marked)


def all_plans(lib, configs=CONFIGS):
    """yields (plan id, full listing) over the whole plan set"""
    for config in configs:
        kw, sd, npts = setup(config)
        for tag, dtype, res in engines_of(config):
            for opts in OPTION_SETS:
                yield f'{config}/{tag}/{option_id(opts)}', listing(lib, kw, sd, npts, dtype, res, opts)
