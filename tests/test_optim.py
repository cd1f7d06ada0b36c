"""achelous_amd/optim.py FusedOptimizer (csrc/k_optim.h; include/achelous_optim.h): the optimizer step and the weight EMA over one flat training-state arena.

Truth is the reference itself: tests/golden/optim_traj.npz / optim_traj.meta.json hold the group membership that train.py:499-518 gives on the reference's models and,
for the variants of tests/optim_cases.py, what `torch.optim.*` + the reference's `ModelEMA` + `set_optimizer_lr` compute in float64 over five steps of seeded gradients
(gen_optim_golden.py) — as the DISPLACEMENT from the initial state, sampled, with torch float32's own deviation as the yardstick.  The smallest shapes are held against
torch's optimizers directly.  Every case runs under the emulation library (`-m "not gpu"`) and on the MI355X (`-m gpu`) unless it is host-only.

Bound (tests/test_train_functional.py's rule and constants): error < min(2e-4, max(2^-20, 8 x yardstick)) in the max-norm relative metric, per class of tensors
(parameters, EMA parameters, EMA float buffers).  gen_optim_golden.py asserts that a dropped decay, a dropped Nesterov term and an extra EMA tick each move the
compared quantity by at least 20 x this bound."""
import copy
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import optim_cases as OC
from achelous_amd import Achelous, engine as E, train_ops
from achelous_amd.optim import CHUNK, H_D, H_LR, H_UPDATES, FusedOptimizer, reference_param_groups
from achelous_amd.synth import condition_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
TOL, FLOOR, F_YARD = 2e-4, 2.0 ** -20, 8
DEVICES = [pytest.param('cpu', id='emu'), pytest.param('cuda', id='gpu', marks=pytest.mark.gpu)]
META = json.load(open(os.path.join(HERE, 'golden', 'optim_traj.meta.json')))


@pytest.fixture(params=DEVICES)
def dev(request):
    """'cpu': the kernels under the emulation library; 'cuda': the HIP kernels"""
    if request.param == 'cpu':
        from emu_util import emu_library
        train_ops._lib.test_library = emu_library()
        try:
            yield 'cpu'
        finally:
            train_ops._lib.test_library = None
    else:
        yield 'cuda'


def _bound(largest, yard_abs):
    return min(TOL, max(FLOOR, F_YARD * yard_abs / largest))


# ---------------------------------------------------------------------------------------------------------------------- 1. groups
@pytest.mark.parametrize('config', list(OC.GROUP_CONFIGS))
def test_reference_param_groups_match_the_reference(config):
    """name for name what train.py:499-518 builds on the reference's own model; 'rv': one group of everything"""
    got = reference_param_groups(Achelous(**OC.GROUP_CONFIGS[config]))
    want = META['groups'][config]
    assert [list(g) for g in got] == want
    if config == 'rv_s0':
        assert len(got[0]) > 0 and got[1:] == ([], [], [])
    if config == 'en_s0_gdf':
        assert [len(g) for g in got] == [80, 212, 213, 26]
        assert {k.rsplit('.', 1)[-1] for k in got[3]} == {'gamma', 'gamma_xca', 'temperature', 'cweight', 'cbias', 'sweight', 'sbias'}


# ---------------------------------------------------------------------------------------------------------------------- 2. trajectories
_fixture = {}


def _traj():
    if not _fixture:
        fx = np.load(os.path.join(HERE, 'golden', 'optim_traj.npz'))
        _fixture.update(names=json.loads(bytes(fx['names::json']).decode()), count=fx['count'], idx=fx['idx'], fx=fx)
    return _fixture


def _model(dev):
    m = Achelous(**OC.CTOR)
    m.load_state_dict(condition_state_dict(m.state_dict(), seed=OC.WEIGHT_SEED))
    return m.train().to(dev)


@pytest.mark.parametrize('variant', list(OC.VARIANTS))
def test_trajectory_against_the_reference_in_float64(variant, dev):
    v, rec, T = OC.VARIANTS[variant], META['variants'][variant], _traj()
    m = _model(dev)
    assert [k for k, _ in m.named_parameters()] == META['param_names'] and [k for k, _ in OC.float_buffers(m)] == META['buffer_names']
    kw = {k: v[k] for k in ('momentum', 'nesterov', 'betas') if k in v}
    groups = 'reference' if v['groups'] == 'reference' else [{'params': list(m.parameters()), 'weight_decay': v['weight_decay']}]
    opt = FusedOptimizer(m, v['kind'], lr=v['lr'], weight_decay=v['weight_decay'], groups=groups, ema=v['u0'] is not None, ema_updates=v['u0'] or 0, **kw)
    start = {k: t.detach().double().cpu().clone() for k, t in m.named_parameters()}
    if opt.ema_model is not None:
        start.update({'ema::' + k: t.detach().double().cpu().clone() for k, t in opt.ema_model.state_dict().items() if t.is_floating_point()})
    lrs = []

    def set_lr(s):
        opt.set_lr(OC.cos_lr(v['lr'], OC.MIN_LR, OC.STEPS, s))
        lrs.append(opt.param_groups[0]['lr'])
    OC.drive(m, opt, set_lr)
    hyper = opt.hyper.cpu()                                               # read back once, at the end
    assert np.allclose(lrs, rec['lr_per_step'], rtol=1e-12, atol=0), (lrs, rec['lr_per_step'])
    assert all(abs(float(hyper[H_LR + g]) - rec['lr_per_step'][-1]) <= 1e-12 * rec['lr_per_step'][-1] for g in range(len(opt.param_groups)))
    if v['u0'] is not None:
        assert float(hyper[H_UPDATES]) == v['u0'] + OC.STEPS
        assert abs(float(hyper[H_D]) - rec['d_per_step'][-1]) <= 1e-12 * rec['d_per_step'][-1], (float(hyper[H_D]), rec['d_per_step'][-1])
    else:
        assert opt.ema_model is None and opt.ema_arena is None
    now = dict(m.named_parameters())
    if opt.ema_model is not None:
        now.update({'ema::' + k: t for k, t in opt.ema_model.state_dict().items()})
    val = T['fx'][variant + '/val']
    pnames = set(META['param_names'])
    worst = {'param_stat': 0.0, 'ema_param_stat': 0.0, 'ema_buffer_stat': 0.0}
    for r, name in enumerate(T['names'][:len(val)]):
        n, cls = int(T['count'][r]), 'param_stat'
        if name.startswith('ema::'):
            cls = 'ema_param_stat' if name[5:] in pnames else 'ema_buffer_stat'
        disp = now[name].detach().double().cpu().reshape(-1).numpy()[T['idx'][r, :n]] - start[name].reshape(-1).numpy()[T['idx'][r, :n]]
        worst[cls] = max(worst[cls], float(np.abs(disp - val[r, :n]).max()))
    for cls, err in worst.items():
        largest, yard = rec[cls][0], rec[cls][1]
        if largest == 0.0:
            continue
        print(f'{variant} {cls}: error {err / largest:.3e}, yardstick {yard / largest:.3e}, bound {_bound(largest, yard):.3e}')
        assert err / largest < _bound(largest, yard), (variant, cls, err / largest, yard / largest)


# ---------------------------------------------------------------------------------------------------------------------- 3. smallest shapes
SMALL = {
    'sgd_nesterov': dict(kind='sgd', momentum=0.937, nesterov=True),
    'sgd_plain_momentum': dict(kind='sgd', momentum=0.9, nesterov=False),
    'sgd_no_momentum': dict(kind='sgd', momentum=0.0, nesterov=False),
    'adam': dict(kind='adam', betas=(0.937, 0.999)),
    'adamw': dict(kind='adamw', betas=(0.9, 0.999)),
}
SMALL_LR, SMALL_WD, SMALL_STEPS, SMALL_U0 = 1e-2, 5e-2, 4, 3000


def _torch_run(case, dtype):
    """four steps of torch's optimizer (foreach=False) and a statement of the reference's EMA in `dtype` -> displacements of the parameters / of the EMA's float entries"""
    c = SMALL[case]
    m = OC.Standin().to(dtype)
    groups = m.groups(SMALL_WD)
    if c['kind'] == 'sgd':
        opt = torch.optim.SGD(groups, lr=SMALL_LR, momentum=c['momentum'], nesterov=c['nesterov'], foreach=False)
    else:
        opt = (torch.optim.Adam if c['kind'] == 'adam' else torch.optim.AdamW)(groups, lr=SMALL_LR, betas=c['betas'], foreach=False)
    floats = lambda: {k: t for k, t in m.state_dict().items() if t.is_floating_point()}       # noqa: E731
    p0 = {k: t.detach().double().clone() for k, t in floats().items()}
    ema = {k: t.detach().clone() for k, t in floats().items()}
    updates = SMALL_U0
    for s in range(SMALL_STEPS):
        for g in opt.param_groups:
            g['lr'] = SMALL_LR * (1 + s)
        m.standin_grads(s)
        opt.step()
        updates += 1
        d = 0.9999 * (1 - math.exp(-updates / 2000))
        with torch.no_grad():
            for k, t in floats().items():                                    # loss/detection_loss.py:456-459
                ema[k] *= d
                ema[k] += (1 - d) * t.detach()
    return ({k: t.detach().double() - p0[k] for k, t in m.named_parameters()}, {k: t.double() - p0[k] for k, t in ema.items()})


def _padding(opt):
    """the padding elements of every arena, concatenated"""
    out = []
    for arena in (opt.state_arena, opt.ema_arena, opt.grad_arena, opt.m1, opt.m2):
        if arena is None:
            continue
        keep = torch.ones(arena.numel(), dtype=torch.bool)
        for t, (a, _) in zip(opt._tensors, opt._slots):
            if a * CHUNK < arena.numel():
                keep[a * CHUNK:a * CHUNK + t.numel()] = False
        out.append(arena.cpu()[keep])
    return torch.cat(out)


@pytest.mark.parametrize('case', list(SMALL))
def test_smallest_shapes_against_torch(case, dev):
    c = SMALL[case]
    truth_p, truth_e = _torch_run(case, torch.float64)
    yard_p, yard_e = _torch_run(case, torch.float32)
    m = OC.Standin().to(dev)
    opt = FusedOptimizer(m, lr=SMALL_LR, weight_decay=SMALL_WD, groups=m.groups(SMALL_WD), ema_updates=SMALL_U0, **c)
    assert len(opt.state) == 0 and [len(g['params']) for g in opt.param_groups] == [4, 3, 2]
    p0 = {k: t.detach().cpu().clone() for k, t in m.state_dict().items()}
    pad0 = _padding(opt)
    assert pad0.numel() > 0 and not pad0.any()
    for s in range(SMALL_STEPS):
        opt.set_lr(SMALL_LR * (1 + s))
        m.standin_grads(s)
        opt.step()
        opt.zero_grad()
    assert torch.equal(_padding(opt).view(torch.int32), pad0.view(torch.int32)), 'a padding element changed'
    for k in ('never', 'loose'):
        assert torch.equal(getattr(m, k).detach().cpu().view(torch.int32), p0[k].view(torch.int32)), f'{k} has no gradient and changed'
    assert int(m.count) == 11 and int(opt.ema_model.count) == 11 and opt.ema_model.count.dtype == torch.int64
    assert not opt.ema_model.training and not any(p.requires_grad for p in opt.ema_model.parameters())
    if c['kind'] != 'sgd':
        assert sorted(set(opt.t.cpu().tolist())) == [0, 2, 4]             # never / loose, late (from step 2 on), every other parameter
    got_p = {k: t.detach().double().cpu() - p0[k].double() for k, t in m.named_parameters()}
    got_e = {k: t.detach().double().cpu() - p0[k].double() for k, t in opt.ema_model.state_dict().items() if t.is_floating_point()}
    for what, got, truth, yard in (('parameters', got_p, truth_p, yard_p), ('ema', got_e, truth_e, yard_e)):
        largest = max(float(t.abs().max()) for t in truth.values())
        err = max(float((got[k] - truth[k]).abs().max()) for k in truth)
        yd = max(float((yard[k] - truth[k]).abs().max()) for k in truth)
        print(f'{case} {what}: error {err / largest:.3e}, yardstick {yd / largest:.3e}, bound {_bound(largest, yd):.3e}')
        assert err / largest < _bound(largest, yd), (case, what, err / largest, yd / largest)


def test_without_ema_no_arena_is_allocated(dev):
    m = OC.Standin().to(dev)
    opt = FusedOptimizer(m, 'sgd', lr=SMALL_LR, groups=m.groups(SMALL_WD), ema=False)
    assert opt.ema_arena is None and opt.ema_model is None and opt.m2 is None and opt.t is None
    before = m.p4.detach().clone()
    m.standin_grads(0)
    opt.step()
    assert not torch.equal(m.p4.detach(), before) and float(opt.hyper[H_UPDATES]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------- 4. plumbing
def test_model_aliases_the_arena_and_versions_move(dev):
    ref = OC.Standin()
    m = OC.Standin().to(dev)
    opt = FusedOptimizer(m, 'sgd', lr=SMALL_LR, groups=m.groups(SMALL_WD))
    lo, hi = opt.state_arena.data_ptr(), opt.state_arena.data_ptr() + 4 * opt.state_arena.numel()
    for (k, t), (_, r) in zip(m.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(t.cpu(), r), k                                                     # values unchanged, bit for bit
        assert (lo <= t.data_ptr() < hi and t.data_ptr() % 1024 == lo % 1024) == t.is_floating_point(), k
    elo, ehi = opt.ema_arena.data_ptr(), opt.ema_arena.data_ptr() + 4 * opt.ema_arena.numel()
    assert all((elo <= t.data_ptr() < ehi) == t.is_floating_point() for t in opt.ema_model.state_dict().values())
    m.standin_grads(0)
    v0 = {k: t._version for k, t in m.named_parameters()}
    e0 = {k: t._version for k, t in opt.ema_model.state_dict().items()}
    opt.step()
    assert all(t._version > v0[k] for k, t in m.named_parameters() if k not in ('never', 'loose'))
    assert all(t._version > e0[k] for k, t in opt.ema_model.state_dict().items() if t.is_floating_point())
    # an in-place load keeps the aliasing and keeps working
    m.load_state_dict({k: (t + 1 if t.is_floating_point() else t) for k, t in ref.state_dict().items()})
    a = opt._slots[0][0] * CHUNK
    assert float(opt.state_arena[a]) == float(opt._tensors[0].detach().reshape(-1)[0]) == float(ref.p0.detach()[0] + 1)
    m.standin_grads(1)
    opt.set_ema_updates(100)                                                                  # the reference's `ema.updates = epoch_step * epoch`
    opt.step()
    assert float(opt.hyper[H_UPDATES]) == 101.0 and abs(float(opt.hyper[H_D]) - 0.9999 * (1 - math.exp(-101 / 2000))) < 1e-13
    # lost aliasing raises
    m.load_state_dict({k: t.to(dev) for k, t in ref.state_dict().items()}, assign=True)
    m.standin_grads(2)
    with pytest.raises(RuntimeError, match='rebuild the optimizer'):
        opt.step()


@pytest.mark.gpu
def test_a_moved_model_raises():
    m = OC.Standin().cuda()
    opt = FusedOptimizer(m, 'sgd', lr=SMALL_LR, groups=m.groups(SMALL_WD))
    m.standin_grads(0)
    opt.step()
    m.to('cpu')
    with pytest.raises(RuntimeError, match='rebuild the optimizer'):
        opt.step()


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_state_dict_round_trip(kind, dev):
    def fresh(seed):
        m = OC.Standin(seed).to(dev)
        return m, FusedOptimizer(m, kind, lr=SMALL_LR, weight_decay=SMALL_WD, groups=m.groups(SMALL_WD), ema_updates=7)
    ma, a = fresh(3)
    for s in range(2):
        a.set_lr(SMALL_LR * (2 + s))
        ma.standin_grads(s)
        a.step()
    sd = copy.deepcopy(a.state_dict())
    mb, b = fresh(4)
    b.load_state_dict(sd)
    for k, t in a._arenas().items():
        if t is not None:
            assert torch.equal(t, b._arenas()[k]) and (t.dtype != torch.float32 or torch.equal(t.view(torch.int32), b._arenas()[k].view(torch.int32))), k
    assert b.param_groups[0]['lr'] == a.param_groups[0]['lr']
    for m, o in ((ma, a), (mb, b)):
        m.standin_grads(2)
        o.step()
    for (k, x), (_, y) in zip(list(ma.state_dict().items()) + list(a.ema_model.state_dict().items()), list(mb.state_dict().items()) + list(b.ema_model.state_dict().items())):
        assert torch.equal(x, y), k
    assert torch.equal(a.hyper, b.hyper)


# ---------------------------------------------------------------------------------------------------------------------- 5. ABI
def test_optim_header_and_binding_tables():
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert E.OPTIM_ENTRIES == {'ach_optim_tick': (ctypes.c_int, [vp, vp]),
                               'ach_optim_step': (ctypes.c_int, [vp] * 8 + [i64, i64, i32, i32, f64, f64, f64, f64, vp])}
    assert len(E.PROTOTYPES) == 88 and not set(E.OPTIM_ENTRIES) & set(E.PROTOTYPES)
    assert set(E.EXTENSIONS) == {'ach_heatmap_frames'} and E.EXTENSION_HEADERS == ('achelous_heatmap.h',) and set(E.POINT_ENTRIES) == {'ach_scatter_points_frames'}
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(E.HEADER), 'achelous_optim.h')).read(), flags=re.S)
    assert re.findall(r'\b(ach_\w+)\s*\(', src) == ['ach_optim_tick', 'ach_optim_step'] and '#include "achelous.h"' in src
    from emu_util import emu_library
    for lib in (emu_library().lib, ctypes.CDLL(E.HIP_LIBRARY)):
        for name in E.OPTIM_ENTRIES:
            assert hasattr(lib, name), name


def test_entry_argument_checks(dev):
    """every ACH_ERR_INVALID case of include/achelous_optim.h through the C entries themselves: nothing is launched, the arenas keep their bytes"""
    m = OC.Standin().to(dev)
    opt = FusedOptimizer(m, 'adam', lr=SMALL_LR, groups=m.groups(SMALL_WD))
    L, P, s = opt._lib.lib, (lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())), ctypes.c_void_p(0)
    good = dict(state=opt.state_arena, ema=opt.ema_arena, grad=opt.grad_arena, m1=opt.m1, m2=opt.m2, flags=opt.flags, t=opt.t, hyper=opt.hyper, chunks=opt.chunks,
                pchunks=opt.param_chunks, kind=1, nesterov=0, momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8)
    before = opt.state_arena.clone()

    def call(**bad):
        a = dict(good, **bad)
        return L.ach_optim_step(P(a['state']), P(a['ema']), P(a['grad']), P(a['m1']), P(a['m2']), P(a['flags']), P(a['t']), P(a['hyper']), a['chunks'], a['pchunks'], a['kind'],
                                a['nesterov'], a['momentum'], a['beta1'], a['beta2'], a['eps'], s)
    for bad in (dict(state=None), dict(grad=None), dict(flags=None), dict(hyper=None), dict(chunks=0), dict(pchunks=0), dict(pchunks=opt.chunks + 1), dict(kind=3), dict(kind=-1),
                dict(m2=None), dict(t=None), dict(m1=None), dict(kind=0, momentum=0.9, m1=None), dict(beta1=1.0), dict(eps=-1.0), dict(state=opt.state_arena[1:])):
        assert call(**bad) == -1, bad
        assert b'ach_optim_step' in L.ach_last_error(None)
    assert L.ach_optim_tick(None, s) == -1
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert torch.equal(opt.state_arena, before)


# ---------------------------------------------------------------------------------------------------------------------- 6. host sanitizers
def test_kernels_under_host_sanitizers(tmp_path):
    """tests/hostemu/optim_main.cpp — k_optim.h against the emulator, arenas of exactly their size, the shapes of case 3 — built with -fsanitize=address,undefined:
    exit 0 and no report.  CPU only, no Python in the process."""
    cxx = shutil.which('g++')
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if cxx is None or subprocess.run([cxx, *san, str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode != 0:
        pytest.skip('the compiler has no sanitizer runtime')
    exe = str(tmp_path / 'optim_main')
    emu, csrc = os.path.join(HERE, 'hostemu'), os.path.join(REPO, 'achelous_amd', 'csrc')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', *san, '-DACH_HOSTEMU', '-I' + emu, '-I' + csrc, '-Wno-unknown-pragmas', os.path.join(emu, 'optim_main.cpp'),
                    os.path.join(emu, 'hostemu.cpp'), '-o', exe, '-lpthread'], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and 'optim_main: ok' in run.stdout and 'ERROR' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-2000:]
