"""Training-mode shared-MLP layer (achelous_amd/train_ops.py, csrc/k_train.h) against torch autograd on the same parameters:
forward, running statistics, and every gradient.  CPU: the kernels under the emulation library; `-m gpu`: the HIP kernels."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from achelous_amd import train_ops


def _reference(cin, cout, relu, seed):
    torch.manual_seed(seed)
    conv, bn = nn.Conv1d(cin, cout, 1), nn.BatchNorm1d(cout)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3); bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
    return conv, bn


def _run(dev, B, cin, cout, N, relu, seed=0, conv_bias=None):
    """Truth = the torch layers in float64, with ONE concession that makes the comparison well-posed: where a BatchNorm output lies within rounding of zero, on which side of it a
    float32 evaluation lands — and with that one whole term of dbeta / dgamma / dW / dx — depends on the summation order of the convolution (33 M outputs in the largest GPU case:
    a handful of such elements, in torch's own float32 kernels as much as in ours).  The truth's backward therefore uses the native layer's ReLU mask, after checking that the two
    masks differ only at elements whose true pre-activation is at rounding distance from zero."""
    layer = train_ops.SharedMLP1d(cin, cout, relu=relu)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, cin, N, generator=g)
    dy = torch.randn(B, cout, N, generator=g)
    layer.conv.load_state_dict(_reference(cin, cout, relu, seed)[0].state_dict()); layer.bn.load_state_dict(_reference(cin, cout, relu, seed)[1].state_dict())
    if conv_bias is not None:
        torch.nn.init.constant_(layer.conv.bias, conv_bias)
    layer = layer.to(dev).train()
    xn = x.clone().to(dev).requires_grad_(True)
    yn = layer(xn)
    yn.backward(dy.to(dev))
    conv, bn = _reference(cin, cout, relu, seed)
    if conv_bias is not None:
        torch.nn.init.constant_(conv.bias, conv_bias)
    conv, bn = conv.double().train(), bn.double().train()
    xr = x.clone().double().requires_grad_(True)
    pre = bn(conv(xr))
    if relu:
        mask = yn.detach().cpu() > 0
        diff = mask != (pre.detach() > 0)
        assert int(diff.sum()) <= max(2, int(2e-6 * diff.numel())) and (not diff.any() or float(pre.detach()[diff].abs().max()) < 2e-5), (int(diff.sum()), diff.numel())
        yr = pre * mask.double()
    else:
        yr = pre
    yr.backward(dy.double())
    truth = {'y': yr.detach(), 'dx': xr.grad, 'dW': conv.weight.grad, 'dgamma': bn.weight.grad, 'dbeta': bn.bias.grad, 'running_mean': bn.running_mean, 'running_var': bn.running_var}
    ours = {'y': yn, 'dx': xn.grad, 'dW': layer.conv.weight.grad, 'dgamma': layer.bn.weight.grad, 'dbeta': layer.bn.bias.grad,
            'running_mean': layer.bn.running_mean, 'running_var': layer.bn.running_var}
    rel = lambda a, b: ((a.detach().cpu().double() - b.detach().double()).abs().max() / (b.detach().double().abs().max() + 1e-12)).item()
    errs = {k: rel(ours[k], truth[k]) for k in truth}
    assert max(errs.values()) < 2e-4, errs
    # the conv bias feeds a training-mode BatchNorm: its true gradient is rounding noise around zero
    assert layer.conv.bias.grad.abs().max().item() == 0.0 and conv.bias.grad.abs().max().item() < 1e-6 * dy.abs().sum().item()
    assert int(layer.bn.num_batches_tracked) == 1
    return errs


SHAPES = [(2, 5, 64, 48, True), (3, 64, 128, 100, True), (2, 128, 1024, 33, True), (4, 160, 100, 20, True), (2, 64, 128, 70, False)]


@pytest.mark.parametrize('B,cin,cout,N,relu', SHAPES)
def test_emulated_shared_mlp_forward_backward_match_autograd(B, cin, cout, N, relu):
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        _run('cpu', B, cin, cout, N, relu)
    finally:
        train_ops._lib.test_library = None


def test_emulated_shared_mlp_with_mean_dominated_pre_activations():
    """A convolution bias of 1000 in front of the BatchNorm: the statistics are taken over values whose mean is a thousand times their spread (a one-pass
    variance E[z^2] - E[z]^2 has no correct digit left in float32 there).  Without the ReLU: a float32 value near 1000 has an ulp of 6e-5, above the 2e-5 within which
    `_run` lets the two ReLU masks differ — with it the case would measure on which side of zero a rounding falls, not the statistics."""
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        print(_run('cpu', 3, 64, 128, 100, False, conv_bias=1000.0))
    finally:
        train_ops._lib.test_library = None


@pytest.mark.gpu
def test_gpu_shared_mlp_with_mean_dominated_pre_activations():
    print(_run('cuda', 64, 5, 64, 512, False, conv_bias=1000.0))


@pytest.mark.gpu
@pytest.mark.parametrize('B,cin,cout,N,relu', SHAPES + [(64, 5, 64, 512, True), (64, 128, 1024, 512, True)])
def test_gpu_shared_mlp_forward_backward_match_autograd(B, cin, cout, N, relu):
    print(_run('cuda', B, cin, cout, N, relu))


@pytest.mark.gpu
def test_gpu_shared_mlp_trains():
    """A few SGD steps on a two-layer stack fit random targets better than at the start (gradients point downhill), and eval mode
    (running statistics) reproduces nn.BatchNorm1d's eval output."""
    torch.manual_seed(0)
    net = nn.Sequential(train_ops.SharedMLP1d(5, 32), train_ops.SharedMLP1d(32, 8, relu=False)).cuda().train()
    x, t = torch.randn(8, 5, 128).cuda(), torch.randn(8, 8, 128).cuda()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = ((net(x) - t) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.8 * losses[0], losses
    net.eval()
    ref = nn.Sequential(nn.Conv1d(5, 32, 1), nn.BatchNorm1d(32), nn.ReLU(), nn.Conv1d(32, 8, 1), nn.BatchNorm1d(8)).cuda().eval()
    ref[0].load_state_dict(net[0].conv.state_dict()); ref[1].load_state_dict(net[0].bn.state_dict())
    ref[3].load_state_dict(net[1].conv.state_dict()); ref[4].load_state_dict(net[1].bn.state_dict())
    with torch.no_grad():
        assert torch.allclose(net(x), ref(x), rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------- Ghost blocks (neck / decoders)
def _torch_ghost(inp, oup, relu):
    init = (oup + 1) // 2
    class G(nn.Module):                                       # ghost_conv.py:6-29 stated with torch layers (the checker)
        def __init__(self):
            super().__init__()
            self.oup = oup
            self.primary_conv = nn.Sequential(nn.Conv2d(inp, init, 1, 1, 0, bias=False), nn.BatchNorm2d(init), nn.ReLU() if relu else nn.Sequential())
            self.cheap_operation = nn.Sequential(nn.Conv2d(init, init, 3, 1, 1, groups=init, bias=False), nn.BatchNorm2d(init), nn.ReLU() if relu else nn.Sequential())
        def forward(self, x):
            x1 = self.primary_conv(x)
            return torch.cat([x1, self.cheap_operation(x1)], 1)[:, :self.oup]
    return G()


def _torch_bottleneck(i, m, o):
    class Bk(nn.Module):                                      # ghost_conv.py:32-70, stride 1
        def __init__(self):
            super().__init__()
            self.ghost1, self.ghost2 = _torch_ghost(i, m, True), _torch_ghost(m, o, False)
            self.shortcut = nn.Sequential() if i == o else nn.Sequential(nn.Conv2d(i, i, 3, 1, 1, groups=i, bias=False), nn.BatchNorm2d(i), nn.Conv2d(i, o, 1, bias=False), nn.BatchNorm2d(o))
        def forward(self, x):
            return self.ghost2(self.ghost1(x)) + self.shortcut(x)
    return Bk()


def _run_module(dev, native, ref, xshape, seed=0):
    torch.manual_seed(seed)
    with torch.no_grad():
        for p_ in ref.parameters():
            p_.copy_(torch.randn_like(p_) * (0.3 if p_.dim() > 1 else 0.2) + (1.0 if p_.dim() == 1 else 0.0))
    native.load_state_dict(ref.state_dict(), strict=True)      # same parameter names as the torch statement of the reference block
    native = native.to(dev).train(); ref.train()
    x = torch.randn(*xshape)
    xr = x.clone().requires_grad_(True); xn = x.clone().to(dev).requires_grad_(True)
    yr = ref(xr); yn = native(xn)
    dy = torch.randn_like(yr)
    yr.backward(dy); yn.backward(dy.to(dev))
    # A BatchNorm shift that feeds a linear layer + another training-mode BatchNorm (shortcut.1.bias) has a true gradient of ZERO:
    # both implementations return rounding noise there.  Errors are therefore measured against max(|reference|, 1e-3 x the largest
    # parameter gradient of the block) — noise in a vanishing gradient is judged on the scale of the gradients around it.
    refp = dict(ref.named_parameters())
    gscale = max(float(p_.grad.abs().max()) for p_ in refp.values())
    def rel(a, b, floor=0.0):
        a, b = a.detach().cpu().double(), b.detach().double()
        return ((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-12)).item()
    errs = {'y': rel(yn, yr), 'dx': rel(xn.grad, xr.grad)}
    for k, v in native.named_parameters():
        errs['d' + k] = rel(v.grad, refp[k].grad, 1e-3 * gscale)
    refb = dict(ref.named_buffers())
    for k, v in native.named_buffers():
        if 'running' in k:
            errs[k] = rel(v, refb[k])
    assert max(errs.values()) < 5e-4, errs
    return errs


GHOST_CASES = [('module', (48, 48, True), (2, 48, 12, 10)), ('module', (32, 9, True), (2, 32, 9, 16)), ('module', (96, 48, False), (1, 96, 8, 8)),
               ('bottleneck', (96, 96, 48), (2, 96, 10, 10)), ('bottleneck', (32, 32, 32), (2, 32, 6, 7)), ('bottleneck', (32, 48, 24), (2, 32, 6, 7))]
# (rows of 10 and 7 take the depthwise kernel with one output per thread, rows of 16 and 8 the one with four; (32, 32, 32) is the identity form, (32, 48, 24) has mid != in)


def _ghost_pair(kind, args):
    if kind == 'module':
        return train_ops.GhostModule(*args), _torch_ghost(*args)
    return train_ops.GhostBottleneck(*args), _torch_bottleneck(*args)


@pytest.mark.parametrize('kind,args,xshape', GHOST_CASES)
def test_emulated_ghost_blocks_forward_backward_match_autograd(kind, args, xshape):
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        _run_module('cpu', *_ghost_pair(kind, args), xshape)
    finally:
        train_ops._lib.test_library = None


@pytest.mark.gpu
@pytest.mark.parametrize('kind,args,xshape', GHOST_CASES[:5] + [('bottleneck', (192, 192, 96), (64, 192, 20, 20)), ('module', (32, 9, True), (8, 32, 320, 320))] + GHOST_CASES[5:])          # (later cases behind the two large ones: the ids of the earlier ones stay)
def test_gpu_ghost_blocks_forward_backward_match_autograd(kind, args, xshape):
    print(_run_module('cuda', *_ghost_pair(kind, args), xshape))


# ---------------------------------------------------------------------------------------- the PointNet branch, end to end
class _TorchSTN(nn.Module):                                   # pointnet_utils.py:10-85 stated with torch layers (the checker)
    def __init__(self, channel, k):
        super().__init__()
        self.k = k
        self.conv1, self.conv2, self.conv3 = nn.Conv1d(channel, 64, 1), nn.Conv1d(64, 128, 1), nn.Conv1d(128, 1024, 1)
        self.fc1, self.fc2, self.fc3 = nn.Linear(1024, 512), nn.Linear(512, 256), nn.Linear(256, k * k)
        self.relu = nn.ReLU()
        self.bn1, self.bn2, self.bn3, self.bn4, self.bn5 = (nn.BatchNorm1d(c) for c in (64, 128, 1024, 512, 256))
    def forward(self, x):
        F = torch.nn.functional
        x = F.relu(self.bn1(self.conv1(x))); x = F.relu(self.bn2(self.conv2(x))); x = F.relu(self.bn3(self.conv3(x)))
        x = torch.max(x, 2, keepdim=True)[0].view(-1, 1024)
        x = F.relu(self.bn4(self.fc1(x))); x = F.relu(self.bn5(self.fc2(x))); x = self.fc3(x)
        return (x + torch.eye(self.k).view(1, -1)).view(-1, self.k, self.k)


class _TorchEncoder(nn.Module):                               # pointnet_utils.py:88-133
    def __init__(self, channel):
        super().__init__()
        self.stn = _TorchSTN(channel, 3)
        self.conv1, self.conv2, self.conv3 = nn.Conv1d(channel, 32, 1), nn.Conv1d(32, 64, 1), nn.Conv1d(64, 128, 1)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(32), nn.BatchNorm1d(64), nn.BatchNorm1d(128)
        self.fstn = _TorchSTN(32, 32)
    def forward(self, x):
        F = torch.nn.functional
        B, D, N = x.size()
        trans = self.stn(x)
        x = x.transpose(2, 1)
        feature, x = x[:, :, 3:], x[:, :, :3]
        x = torch.cat([torch.bmm(x, trans), feature], dim=2).transpose(2, 1)
        x = F.relu(self.bn1(self.conv1(x)))
        trans_feat = self.fstn(x)
        x = torch.bmm(x.transpose(2, 1), trans_feat).transpose(2, 1)
        pointfeat = x
        x = F.relu(self.bn2(self.conv2(x)))
        x = self.bn3(self.conv3(x))
        x = torch.max(x, 2, keepdim=True)[0].view(-1, 128)
        return torch.cat([x.view(-1, 128, 1).repeat(1, 1, N), pointfeat], 1), trans, trans_feat


class _TorchPointNetSeg(nn.Module):                           # pointnet_sem_seg.py:13-37
    def __init__(self, k, channel):
        super().__init__()
        self.k = k
        self.feat = _TorchEncoder(channel)
        self.conv1, self.conv2, self.conv3, self.conv4 = nn.Conv1d(160, 128, 1), nn.Conv1d(128, 100, 1), nn.Conv1d(100, 64, 1), nn.Conv1d(64, k, 1)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(128), nn.BatchNorm1d(100), nn.BatchNorm1d(64)
    def forward(self, x):
        F = torch.nn.functional
        B, n_pts = x.size(0), x.size(2)
        x, _, _ = self.feat(x)
        x = F.relu(self.bn1(self.conv1(x))); x = F.relu(self.bn2(self.conv2(x))); x = F.relu(self.bn3(self.conv3(x)))
        x = self.conv4(x).transpose(2, 1).contiguous()
        return F.log_softmax(x.view(-1, self.k), dim=-1).view(B, n_pts, self.k)


def _run_pointnet(dev, B, N, seed=0):
    """Truth = the torch statement in FLOAT64.  Two things make an end-to-end fp32 comparison of this network soft, for torch's own
    fp32 evaluation as much as for ours: BatchNorm over a handful of samples (the STN's fc layers normalise over the batch: torch fp32
    deviates from fp64 by 1-5 % on some gradients at B = 4..16), and the three max-over-points — with 8 k rows of 128-512 points a
    near-tie within fp32 rounding happens in a fair share of runs, and whichever implementation resolves it differently from fp64
    routes that row's gradient to another point (one row of one weight gradient moves by ~1 / B; measured 11 % in max-norm on one
    row, 0.3 % of the matrix in L2).  Every layer is compared tightly on its own above; here the metric is the relative L2 error per
    tensor, bound max(5e-2, 2 x torch-fp32's own deviation): a resolved-differently tie moves the first layers' gradients by up to ~1 % in L2
    (seed 0 at B = 8: ours 0.8 %, torch 0.001 %; seed 1: ours 0.001 %, torch 0.2 %; MI355X at B = 16, N = 512: ours 1.7 %, torch 0.2 %); a wiring error moves them by O(1)."""
    import copy
    torch.manual_seed(seed)
    ref = _TorchPointNetSeg(8, 5)
    native = train_ops.PointNetSeg(8, 5)
    assert list(native.state_dict().keys()) == list(ref.state_dict().keys())
    native.load_state_dict(ref.state_dict(), strict=True)
    ref64 = copy.deepcopy(ref).double().train()
    native = native.to(dev).train(); ref.train()
    x = torch.randn(B, 5, N) * 0.5
    target = torch.randint(0, 8, (B, N))
    nll = torch.nn.functional.nll_loss

    def run(model, xin, d):
        xx = xin.clone().to(d).requires_grad_(True)
        y = model(xx)
        loss = nll(y.reshape(-1, 8), target.reshape(-1).to(d))
        loss.backward()
        g = {'d' + k: v.grad.detach().cpu().double() for k, v in model.named_parameters()}
        g.update({k: v.detach().cpu().double() for k, v in model.named_buffers() if 'running' in k})
        g.update({'log_probs': y.detach().cpu().double(), 'dx': xx.grad.detach().cpu().double(), 'loss': loss.detach().cpu().double().reshape(1)})
        return g
    truth, t32, nat = run(ref64, x.double(), 'cpu'), run(ref, x, 'cpu'), run(native, x, dev)
    gscale = max(float(v.abs().max()) for k, v in truth.items() if k.startswith('d') and k != 'dx')
    worst = (None, 0.0, 0.0)
    for k, tv in truth.items():
        floor = 1e-3 * gscale * tv.numel() ** 0.5 if k.startswith('d') else 0.0   # vanishing gradients (a bias in front of a BatchNorm): judged on the gradient scale
        den = max(float(tv.norm()), floor, 1e-12)
        e_nat, e_t32 = float((nat[k] - tv).norm()) / den, float((t32[k] - tv).norm()) / den
        assert e_nat < max(5e-2, 2.0 * e_t32), (k, e_nat, e_t32)
        if e_nat > worst[1]:
            worst = (k, e_nat, e_t32)
    return {'worst tensor': worst[0], 'native vs fp64': worst[1], 'torch fp32 vs fp64 there': worst[2]}


def test_emulated_pointnet_branch_trains_natively_end_to_end():
    """The whole `pc_seg_model` (STN3d, STNkd, encoder, head: 60 parameter tensors, 1.9 M parameters) forward + backward on the
    native kernels against the same network stated with torch layers: log-probabilities, the loss, the input gradient, every
    parameter gradient and every running statistic."""
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        print(_run_pointnet('cpu', 4, 64))
    finally:
        train_ops._lib.test_library = None


@pytest.mark.gpu
def test_gpu_pointnet_branch_trains_natively_end_to_end():
    print(_run_pointnet('cuda', 16, 512))


def test_pointnet_seg_state_dict_is_the_reference_pc_seg_model():
    """`train_ops.PointNetSeg` registers exactly the `pc_seg_model.*` entries (names, shapes, order) captured from the imported
    reference (tests/golden/en_s0.keys.json): a reference checkpoint's point branch loads into it unchanged."""
    import json
    import os
    from golden_util import GOLDEN_DIR
    meta = json.load(open(os.path.join(GOLDEN_DIR, 'en_s0.keys.json')))
    ref = [(k[len('pc_seg_model.'):], tuple(s)) for k, s, _ in meta['keys'] if k.startswith('pc_seg_model.')]
    mine = [(k, tuple(v.shape)) for k, v in train_ops.PointNetSeg(8, 5).state_dict().items()]
    assert len(ref) == 118 and ref == mine


# ---------------------------------------------------------------------------------------- eval mode of the stand-alone blocks; the model's branch through the stand-alone module
def _run_eval(dev, native, ref, xshape, seed=0):
    """`.eval()` under no_grad — the running-statistics branch of the shared evaluator — against the torch statement in float64 `.eval()`, with conditioned running
    statistics (not the 0 / 1 defaults).  Bound: tests/test_train_functional.py's rule max(FLOOR, F_YARD x yardstick), the yardstick being torch's float32 `.eval()` of the
    same module against the same truth.  The BatchNorm counters stay where they are in eval mode and move by exactly 1 per training forward."""
    import copy
    import test_train_functional as P
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in ref.named_buffers():
            if k.endswith('running_mean'):
                v.copy_(torch.randn(v.shape, generator=g) * 0.1)
            if k.endswith('running_var'):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    native.load_state_dict(ref.state_dict(), strict=True)
    truth, native, ref = copy.deepcopy(ref).double().eval(), native.to(dev).eval(), ref.eval()
    x = torch.randn(*xshape, generator=g) * 0.5
    counters = lambda: [int(v) for k, v in native.named_buffers() if k.endswith('num_batches_tracked')]
    before = counters()
    assert len(before) > 0
    with torch.no_grad():
        yt, yf, yn = truth(x.double()), ref(x), native(x.to(dev))
    assert counters() == before
    err, yard = P._rel(yn, yt), P._rel(yf, yt)
    bound = max(P.FLOOR, P.F_YARD * yard)
    print(f'eval {type(native).__name__}{tuple(xshape)} on {dev}: native {err:.3e}, torch float32 {yard:.3e}, bound {bound:.3e}')
    assert err < bound, (err, yard, bound)
    native.train()
    for n in (1, 2):
        native(x.to(dev))
        assert counters() == [c + n for c in before]


EVAL_CASES = {'bottleneck': (lambda: (train_ops.GhostBottleneck(32, 48, 24), _torch_bottleneck(32, 48, 24)), (2, 32, 6, 7)),
              'pointnet': (lambda: (train_ops.PointNetSeg(8, 5), _TorchPointNetSeg(8, 5)), (2, 5, 16))}


@pytest.mark.parametrize('name', list(EVAL_CASES))
def test_emulated_blocks_in_eval_mode_use_the_running_statistics(name):
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        torch.manual_seed(0)
        _run_eval('cpu', *EVAL_CASES[name][0](), EVAL_CASES[name][1])
    finally:
        train_ops._lib.test_library = None


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(EVAL_CASES))
def test_gpu_blocks_in_eval_mode_use_the_running_statistics(name):
    torch.manual_seed(0)
    _run_eval('cuda', *EVAL_CASES[name][0](), EVAL_CASES[name][1])


def _model_step_through_pointnet_seg(dev):
    """One whole-model training step (tests/test_train_graph.py::_step) and the stand-alone `PointNetSeg` carrying the model's `pc_seg_model.*` state dict, on the same
    points and cotangent: bit-identical log-probabilities and parameter gradients — both are ONE statement of the branch (train_graph.Layers.pointnet)."""
    import test_train_graph as G
    from achelous_amd.synth import make_inputs
    meta, _, m, outs, _ = G._step(dev)
    pfx = 'pc_seg_model.'
    alone = train_ops.PointNetSeg(meta['ctor']['pc_classes'], meta['ctor']['pc_channels'])
    alone.load_state_dict({k[len(pfx):]: v for k, v in m.state_dict().items() if k.startswith(pfx)}, strict=True)
    alone = alone.to(dev).train()
    xp = make_inputs(meta['batch'], meta['input_seed'], resolution=meta['ctor']['resolution'], num_points=meta['num_points'], pc_channels=meta['ctor']['pc_channels'],
                     radar_cells=meta['radar_cells'])[2]
    g = torch.Generator().manual_seed(meta['cotangent_seed'])
    cot = [torch.randn(o.shape, generator=g, dtype=torch.float64).float().to(dev) for o in outs][-1]
    pc = alone(xp.to(dev))
    (pc * cot).sum().backward()
    assert torch.equal(pc, outs[-1])
    theirs = {k[len(pfx):]: v for k, v in m.named_parameters() if k.startswith(pfx)}
    mine = dict(alone.named_parameters())
    assert list(mine) == list(theirs) and len(mine) == 70
    for k, v in mine.items():
        assert torch.equal(v.grad, theirs[k].grad), k


def test_emulated_model_step_and_stand_alone_pointnet_are_one_code_path():
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        _model_step_through_pointnet_seg('cpu')
    finally:
        train_ops._lib.test_library = None


@pytest.mark.gpu
def test_gpu_model_step_and_stand_alone_pointnet_are_one_code_path():
    _model_step_through_pointnet_seg('cuda')


# ---------------------------------------------------------------------------------------- both sides of every shape-dependent dispatch of the C entries
def _dispatch_cases(dev):
    """The smallest shapes on either side of the predicates the C entries (csrc/api_train.cpp) choose a kernel by, each against torch autograd with the check and the
    bounds of tests/test_train_functional.py (`_check`: float64 truth, float32 yardstick, 2e-4 at most):
      four elements per thread or one — a count that divides by four on 16-byte aligned pointers, a count that does not, and the aligned count on a view one float in;
      depthwise k = 3 / 5 / 7 / 9 (unrolled) and 11 (the generic kernels, forward and weight gradient) on a row of 8 (four outputs per thread) and of 6 (one);
      a per-channel reduction in one slice and, above 32 768 values per channel, in two: BatchNorm, LayerNorm's parameter gradients, the depthwise weight gradient."""
    import torch.nn.functional as F
    import test_train_functional as P
    from achelous_amd import train_functional as TF
    one_in = lambda f: (lambda x: f(torch.cat([x.new_zeros(1), x.reshape(-1)])[1:].view(x.shape)))          # the same values, 4 bytes past a 16-byte boundary
    for name, n, wrap in (('n=8', 8, lambda f: f), ('n=6', 6, lambda f: f), ('n=8 one float in', 8, one_in)):
        yield f'act {name}', (lambda n=n, wrap=wrap: P._check(wrap(lambda x: TF.act(x, TF.ACT_SILU)), F.silu, [(P._r(n, scale=2), True)], dev))
    for k in (3, 5, 7, 9, 11):
        for W in (8, 6):
            yield f'dwconv k{k} W{W}', (lambda k=k, W=W: P._check(TF.dwconv, P._ref_dw, [(P._r(1, 2, 5, W), True), (P._r(2, 1, k, k, seed=1, scale=0.3), True), (P._r(2, seed=2), True)], dev))
    for hw in (8, 128):
        shape = (2, 2, hw, hw)
        yield f'batchnorm {shape}', (lambda shape=shape: P._check(lambda x, g, b: TF.batchnorm(x, g, b, None, None, True, 0.1, 1e-5, False), P._ref_bn, [(P._r(*shape), True)] + P._affine(2), dev))
        yield f'layernorm {shape}', (lambda shape=shape: P._check(lambda x, g, b: TF.layernorm_channels(x, g, b, 1e-6), P._ref_ln, [(P._r(*shape), True)] + P._affine(2), dev))
        yield f'dwconv k3 {shape}', (lambda shape=shape: P._check(TF.dwconv, P._ref_dw, [(P._r(*shape), True), (P._r(2, 1, 3, 3, seed=1, scale=0.3), True), (P._r(2, seed=2), True)], dev))


DISPATCH_NAMES = [n for n, _ in _dispatch_cases('cpu')]


@pytest.mark.parametrize('name', DISPATCH_NAMES)
def test_emulated_dispatch_sides_match_autograd(name):
    from emu_util import emu_library
    train_ops._lib.test_library = emu_library()
    try:
        dict(_dispatch_cases('cpu'))[name]()
    finally:
        train_ops._lib.test_library = None


@pytest.mark.gpu
@pytest.mark.parametrize('name', DISPATCH_NAMES)
def test_gpu_dispatch_sides_match_autograd(name):
    dict(_dispatch_cases('cuda'))[name]()
