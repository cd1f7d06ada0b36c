"""Stand-alone training blocks: `nn.Module`s that HOLD the parameters of a reference block under its state-dict keys and evaluate it on the native forward / backward
kernels.

    SharedMLP1d(cin, cout, relu=True)(x)  ==  relu(BatchNorm1d(cout)(Conv1d(cin, cout, 1)(x)))        x [B, cin, N]
    (pointnet_utils.py:29-31, 69-71, 124-127; pointnet_sem_seg.py:31-33 — twelve of PointNet's layers; 1.9 M of the model's 3.6 M parameters)

    GhostModule(inp, oup, relu)(x), GhostBottleneck(in_chs, mid_chs, out_chs)(x)                       x [B, inp, H, W]
    (backbone/conv_utils/ghost_conv.py: `GhostModule` :6-29, `GhostBottleneck` :32-70, stride 1)

    PointNetSeg(num_class, channels)(x)  — the model's `pc_seg_model`                                  x [B, channels, N]

The layers themselves are stated ONCE, in train_graph.py's `Layers` — the evaluator `Achelous.forward` runs in `.train()`: each `forward` below builds it over the
module's own parameters, calls the one method and moves the BatchNorm counters, so a block on its own runs the very code and kernels it runs inside the model.  In
training mode that is batch statistics with `running_mean` / `running_var` updated exactly as nn.BatchNorm does (eps 1e-5, momentum 0.1 — the evaluator's constants for
these layers, which are the values the blocks are built with; a value poked into a block's `.bn` afterwards is not seen), in eval mode the running statistics.  Only
`SharedMLP1d`, the module face of the fused conv + BatchNorm primitive, has its own `forward` and takes `eps` / `momentum`.  The autograd primitives live in
train_functional.py; the underscore names this module re-exports are aliases kept for tests and profiles/scripts.  fp32 on GPU tensors only; no PyTorch-op or CPU fallback.
"""
import torch.nn as nn

from . import train_functional as TF
from ._native import lib as _lib, check as _check, ptr as _p, stream as _stream      # (under these names for tests and profiles/scripts: the definitions are _native's)
from .train_functional import set_gemm_precision, _SharedMLP1dFn, _LinearFn, _BmmPointsFn, _MaxPointsFn, _LogSoftmaxPointsFn      # (likewise: train_functional's)
from .train_graph import Layers


def _evaluate(module, layer, *args):
    """one layer of the evaluator over `module`'s own parameters, in its mode; the BatchNorm counters it went through move at the end"""
    g = Layers(module, module.training)
    y = getattr(g, layer)(*args)
    g.flush_counters()
    return y


class SharedMLP1d(nn.Module):
    """Conv1d(cin, cout, 1) + BatchNorm1d(cout) [+ ReLU] with native forward / backward kernels; state-dict keys `conv.*`, `bn.*`."""

    def __init__(self, cin, cout, relu=True, eps=1e-5, momentum=0.1):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, 1)
        self.bn = nn.BatchNorm1d(cout, eps=eps, momentum=momentum)
        self.relu = relu

    def forward(self, x):
        bn = self.bn
        if self.training and bn.track_running_stats:
            bn.num_batches_tracked += 1
        return TF.shared_mlp(x, self.conv.weight, self.conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.training, bn.momentum, bn.eps, self.relu)


class GhostModule(nn.Module):
    """backbone/conv_utils/ghost_conv.py:6-29 (kernel_size 1, ratio 2, dw_size 3, stride 1) with the reference's parameter names
    (`primary_conv.0/.1`, `cheap_operation.0/.1`); forward / backward run on the native kernels."""

    def __init__(self, inp, oup, relu=True):
        super().__init__()
        self.oup, self.relu = oup, relu
        init = (oup + 1) // 2
        self.primary_conv = nn.Sequential(nn.Conv2d(inp, init, 1, 1, 0, bias=False), nn.BatchNorm2d(init), nn.ReLU(inplace=True) if relu else nn.Sequential())
        self.cheap_operation = nn.Sequential(nn.Conv2d(init, init, 3, 1, 1, groups=init, bias=False), nn.BatchNorm2d(init),
                                             nn.ReLU(inplace=True) if relu else nn.Sequential())

    def forward(self, x):
        return _evaluate(self, 'ghost', x, '', self.oup, self.relu)


class GhostBottleneck(nn.Module):
    """ghost_conv.py:32-70, stride 1 (the only form the Ghost-Dual-FPN uses, neck/ghostdualfpn.py:108-112)."""

    def __init__(self, in_chs, mid_chs, out_chs):
        super().__init__()
        self.mid_chs, self.out_chs = mid_chs, out_chs
        self.ghost1 = GhostModule(in_chs, mid_chs, relu=True)
        self.ghost2 = GhostModule(mid_chs, out_chs, relu=False)
        self.identity = in_chs == out_chs
        self.shortcut = nn.Sequential() if self.identity else nn.Sequential(
            nn.Conv2d(in_chs, in_chs, 3, 1, 1, groups=in_chs, bias=False), nn.BatchNorm2d(in_chs),
            nn.Conv2d(in_chs, out_chs, 1, 1, 0, bias=False), nn.BatchNorm2d(out_chs))

    def forward(self, x):
        return _evaluate(self, 'ghost_bottleneck', x, '', self.out_chs, self.mid_chs)


# ---------------------------------------------------------------------------------------------- PointNet branch, trainable end to end
class _STN(nn.Module):
    """The parameters of STN3d / STNkd (pointnet_utils.py:10-85), under the reference's names; evaluated by `Layers.stn`."""

    def __init__(self, channel, k):
        super().__init__()
        self.k = k
        self.conv1, self.conv2, self.conv3 = nn.Conv1d(channel, 64, 1), nn.Conv1d(64, 128, 1), nn.Conv1d(128, 1024, 1)
        self.fc1, self.fc2, self.fc3 = nn.Linear(1024, 512), nn.Linear(512, 256), nn.Linear(256, k * k)
        self.relu = nn.ReLU()
        self.bn1, self.bn2, self.bn3, self.bn4, self.bn5 = (nn.BatchNorm1d(c) for c in (64, 128, 1024, 512, 256))


class _Encoder(nn.Module):
    """The parameters of PointNetEncoder(global_feat=False, feature_transform=True) (pointnet_utils.py:88-133); evaluated inside `Layers.pointnet`."""

    def __init__(self, channel):
        super().__init__()
        self.stn = _STN(channel, 3)
        self.conv1, self.conv2, self.conv3 = nn.Conv1d(channel, 32, 1), nn.Conv1d(32, 64, 1), nn.Conv1d(64, 128, 1)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(32), nn.BatchNorm1d(64), nn.BatchNorm1d(128)
        self.fstn = _STN(32, 32)


class PointNetSeg(nn.Module):
    """`PointNet_SEG` (nets/pointcloudseg/pointnet2/pointnet_sem_seg.py:13-37) — the `pc_seg_model` of Achelous, 1.9 M of its 3.6 M
    parameters — with the reference's state-dict keys, trainable END TO END on the native kernels: every conv / linear (+ BatchNorm
    in batch-statistics mode + ReLU), the two max-over-points, the two per-sample transforms and the log-softmax run hand-written
    forward and backward kernels; what torch does in between is tensor plumbing (slices, cat / expand, the + identity) whose
    gradients autograd routes.  x [B, channels, N] fp32 -> log-probabilities [B, N, num_class]."""

    def __init__(self, num_class, point_cloud_channels):
        super().__init__()
        self.k = num_class
        self.feat = _Encoder(point_cloud_channels)
        self.conv1, self.conv2, self.conv3, self.conv4 = nn.Conv1d(160, 128, 1), nn.Conv1d(128, 100, 1), nn.Conv1d(100, 64, 1), nn.Conv1d(64, num_class, 1)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(128), nn.BatchNorm1d(100), nn.BatchNorm1d(64)

    def forward(self, x):
        return _evaluate(self, 'pointnet', x, '')
