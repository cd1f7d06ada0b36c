"""The row-tile-resident LayerNorm-prologue GEMMs of the 16-bit engines (achelous_amd/csrc/k_lngemm.h): EdgeNeXt's three patchify convs with the per-tap LayerNorm of
their input pixels and the LayerNorm + qkv projections in front of the cross-covariance attention read and normalise a 16-row tile once — in registers, or through LDS
with the N-chunks dealt to the waves of the tile's workgroup — instead of once per chunk slice.  The same products and the same sums in the same order as gemm_body
(k_gemm.h), so on the CPU emulation every tap behind these launches and every network output has the bits the commit before the change computed
(tests/golden/ln_gemm_parent.*, written by tests/golden/gen_ln_gemm_parent.py on that commit); on the GPU the default plan is held against the separate LayerNorm
launches (ds_fuse = 0) and against the fp32 engine at the bounds of tests/test_gpu_parity.py."""
import json

import numpy as np
import pytest
import torch

import ln_gemm_cases as LC
from emu_util import emu_library

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with open(LC.FIXTURE_JSON) as f:
            _fixture = (json.load(f)['sha256'], np.load(LC.FIXTURE_NPZ))
    return _fixture


@pytest.mark.parametrize('storage', list(LC.STORAGE))
@pytest.mark.parametrize('name,res,batch', LC.CASES)
def test_emulated_taps_and_outputs_have_the_parents_bits(name, res, batch, storage):
    sha, whole = fixture()
    cid = LC.case_id(name, res, batch, storage)
    got, launches = LC.run(emu_library(), name, res, batch, storage)
    # the plan is the production one: the LayerNorm lives in the three patchify convs, the attention is the four-launch form with its own qkv GEMM
    assert sum(n.endswith('.ln+conv') for n in launches) == 3 and sum(n.endswith('.xca.qkv') for n in launches) == 3
    assert set(got) == set(LC.TAPS + LC.OUTPUTS) == set(sha[cid])
    n_whole = 0
    for k in LC.TAPS + LC.OUTPUTS:
        key = cid + '::' + k
        if key in whole.files:
            n_whole += 1
            assert torch.equal(got[k], torch.from_numpy(whole[key])), (cid, k)
        assert LC.digest(got[k]) == sha[cid][k], (cid, k)
    assert n_whole >= 8


# ---- GPU: the same three shapes through the drop-in module
def _gpu_model(name, res):
    from achelous_amd import Achelous
    from achelous_amd.synth import condition_state_dict
    from golden_util import Golden, ctor_kwargs
    g = Golden(name)
    kw = dict(ctor_kwargs(g.meta), resolution=res)
    m = Achelous(**kw).eval()
    m.load_state_dict(g.calibrate(condition_state_dict(m.state_dict(), seed=g.meta['weight_seed'])), strict=True)
    return m.cuda(), kw


@pytest.mark.gpu
@pytest.mark.parametrize('name,res,batch', LC.CASES)
def test_gpu_default_plan_against_separate_layernorms_and_fp32(name, res, batch):
    from achelous_amd.synth import make_inputs
    from test_gpu_parity import H16_TOL, OUTPUTS, _rel
    m, kw = _gpu_model(name, res)
    x, xr, xp = make_inputs(batch, 7, resolution=res, pc_channels=kw['pc_channels'])
    ds_taps = ('backbone.ds1', 'backbone.ds2', 'backbone.ds3')
    with torch.no_grad():
        xs = tuple(t.cuda().bfloat16() for t in (x, xr, xp))
        # the fp32 parity engine (gemm_body) on the tensors the 16-bit engine receives: what the rounding of the INPUTS to bf16 does to the outputs is no property of
        # the engine (tests/test_gpu_parity.py adds it to H16_TOL where the truth is computed from the un-rounded inputs; EN-S2 at 64 x 64, flat H16_TOL against the
        # un-rounded inputs: lane_seg 3.2e-2, the other five outputs 0.2 - 1.1e-2)
        truth = m(*(t.float() for t in xs))
        fused = m(*xs)
        e = m.native_engine(torch.bfloat16)
        names = [o['op'] for o in e.op_table_full()]
        assert sum(n.endswith('.ln+conv') for n in names) == 3 and sum(n.endswith('.xca.qkv') for n in names) == 3
        fused = [t.clone() for t in (*fused[0], fused[1], fused[2], fused[3])]
        fused_taps = {t: e.read_tap(t) for t in ds_taps}
        e.set_option('ds_fuse', 0)
        e.plan(batch)
        plain = m(*xs)
        plain = [t.clone() for t in (*plain[0], plain[1], plain[2], plain[3])]
        plain_taps = {t: e.read_tap(t) for t in ds_taps}
        torch.cuda.synchronize()
        e.set_option('ds_fuse', 1)
        e.plan(batch)
    truth = (*truth[0], truth[1], truth[2], truth[3])
    errs = {k: (_rel(a.float(), t), _rel(a.float(), b.float())) for k, a, b, t in zip(OUTPUTS, fused, plain, truth)}
    tap_errs = {t: _rel(fused_taps[t], plain_taps[t]) for t in ds_taps}
    print(f'{name}/{res}/b{batch}: rel err (vs fp32, vs ds_fuse = 0):', {k: f'{a:.1e} {b:.1e}' for k, (a, b) in errs.items()}, '| taps vs ds_fuse = 0:', {k: f'{v:.1e}' for k, v in tap_errs.items()})
    for k, (vs_truth, vs_plain) in errs.items():
        assert vs_truth < H16_TOL[k], (k, vs_truth)
        assert vs_plain <= 2.0 * H16_TOL[k], (k, vs_plain)
    # the patchify convs themselves: the normalised pixel is rounded to the storage type once on both paths (option ds_fuse: the same arithmetic)
    for t, v in tap_errs.items():
        assert v <= 2.0 * min(H16_TOL.values()), (t, v)
