"""A plain-torch float64 restatement of the RepViT backbone alone (repvit_m1 / m2 / m3 for S0 / S1 / S2), in the FOLDED form the engine runs, written
from the architecture description — so it pins the plan-time folds as well as the network:

    BatchNorm (eps 1e-5) as y = s x + t:  s = gamma / sqrt(var + eps),  t = beta - mean s
    features[0]   : conv3x3 s2 p1 (3 -> C0/2), rows scaled by s, bias t;  erf GELU;  conv3x3 s2 p1 (C0/2 -> C0) likewise
    stride-1 block: d = dw3x3(x; s_conv w3x3, centre tap + s_conv1 w1x1 + 1) + (t_conv + t_conv1)            (RepVGGDW as ONE depthwise conv)
                    d = d * sigmoid(fc2(relu(fc1(mean_hw(d)))))          only in SE rows; fc1 / fc2 with bias, reduced width from fc1.weight
                    y = d + W2' GELU(W1' d + b1') + b2'                  1x1 convs with their BatchNorms folded, hidden 2C
    stride-2 block: t = dw3x3 s2 p1 (x; s w) + t_bn;  t = W' t + b' (inp -> oup);  y = t + W2' GELU(W1' t + b1') + b2'
    maps          : features[i] for i in REPVIT[phi]['out'] — not the stage ends; blocks behind the last one are not run

tests/golden/gen_rv_golden.py asserts it against the imported reference on all four maps and every block output of every fixture configuration
(relative max-norm <= 1e-5); the tests use it as the truth for shapes and weights that have no fixture."""
import torch
import torch.nn.functional as F

from achelous_amd.spec import REPVIT, WIDTHS, repvit_rows

PREFIX = 'image_radar_encoder.fpn.backbone.'
EPS = 1e-5


def bn_st(p, pfx):
    s = p[pfx + '.weight'] / torch.sqrt(p[pfx + '.running_var'] + EPS)
    return s, p[pfx + '.bias'] - p[pfx + '.running_mean'] * s


def conv_bn(p, pfx):
    """Conv2d_BN folded: (weight with rows scaled by s, bias t)"""
    s, t = bn_st(p, pfx + '.bn')
    return p[pfx + '.c.weight'] * s.view(-1, 1, 1, 1), t


def repvgg_dw(p, pfx):
    """RepVGGDW folded to one depthwise 3x3 + bias"""
    w, b = conv_bn(p, pfx + '.conv')
    s1, t1 = bn_st(p, pfx + '.conv1.bn')
    w = w.clone()
    w[:, 0, 1, 1] += s1 * p[pfx + '.conv1.c.weight'].reshape(-1) + 1.0
    return w, b + t1


def se_gate(p, pfx, d):
    """[B, C] gate of timm's SqueezeExcite"""
    m = d.mean((2, 3))
    w1, w2 = p[pfx + '.fc1.weight'], p[pfx + '.fc2.weight']
    h = F.relu(m @ w1.reshape(w1.shape[0], -1).t() + p[pfx + '.fc1.bias'])
    return torch.sigmoid(h @ w2.reshape(w2.shape[0], -1).t() + p[pfx + '.fc2.bias'])


def repvit_forward(state_dict, image, phi, prefix=PREFIX, blocks=None, gates=None):
    """The four backbone maps [B, C_i, H_i, W_i] in float64.  `blocks` (optional dict) receives every features[i] that runs as 'f<i>', `gates` every SE gate."""
    p = {k[len(prefix):]: v.detach().double() for k, v in state_dict.items() if k.startswith(prefix) and v.is_floating_point()}
    out = REPVIT[phi]['out']
    w, b = conv_bn(p, 'features.0.0')
    x = F.gelu(F.conv2d(image.double(), w, b, stride=2, padding=1))
    w, b = conv_bn(p, 'features.0.2')
    x = F.conv2d(x, w, b, stride=2, padding=1)
    assert x.shape[1] == WIDTHS[phi][0]
    if blocks is not None:
        blocks['f0'] = x
    maps = []
    for i, (inp, oup, stride, se) in enumerate(repvit_rows(phi), 1):
        if i > out[-1]:
            break
        f = f'features.{i}.'
        if stride == 2:
            w, b = conv_bn(p, f + 'token_mixer.0')
            d = F.conv2d(x, w, b, stride=2, padding=1, groups=inp)
            w, b = conv_bn(p, f + 'token_mixer.2')
            d = F.conv2d(d, w, b)
        else:
            w, b = repvgg_dw(p, f + 'token_mixer.0')
            d = F.conv2d(x, w, b, padding=1, groups=inp)
            if se:
                g = se_gate(p, f + 'token_mixer.1', d)
                if gates is not None:
                    gates[f'f{i}'] = g
                d = d * g[:, :, None, None]
        w1, b1 = conv_bn(p, f + 'channel_mixer.m.0')
        w2, b2 = conv_bn(p, f + 'channel_mixer.m.2')
        x = d + F.conv2d(F.gelu(F.conv2d(d, w1, b1)), w2, b2)
        if blocks is not None:
            blocks[f'f{i}'] = x
        if i in out:
            maps.append(x)
    return maps
