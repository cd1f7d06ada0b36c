"""A plain-torch float64 restatement of the PoolFormer backbone alone (poolformer_S0 / S1 / S2 with fork_feat: four output norms,
no classifier tail), written from the architecture description:

    x0 = conv7x7 s4 p2 (3 -> C0, bias)
    stage i (i = 0..3), depth[i] blocks:
        y = x + ls1 * ( avgpool3x3_s1_p1_count_include_pad_False(GN1(x)) - GN1(x) )
        z = y + ls2 * fc2( GELU( fc1( GN2(y) ) ) )              1x1 convs, hidden 4C, erf GELU
    out_i = GN_fork_i(x after stage i)                           norm0 / norm2 / norm4 / norm6
    between stages: conv3x3 s2 p1 (C_i -> C_{i+1}, bias) on the UN-normalised stage output
    GN = GroupNorm(1, C), eps 1e-5: mean / biased variance per SAMPLE over C*H*W, affine per channel

tests/golden/gen_pf_golden.py asserts it against the imported reference on all four maps of every fixture configuration (bound
1e-5); the tests use it as the truth for shapes that have no fixture."""
import torch
import torch.nn.functional as F

from achelous_amd.spec import POOLFORMER, WIDTHS

PREFIX = 'image_radar_encoder.fpn.backbone.'


def group_norm1(x, w, b, eps=1e-5):
    mu = x.mean(dim=(1, 2, 3), keepdim=True)
    var = ((x - mu) ** 2).mean(dim=(1, 2, 3), keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def poolformer_forward(state_dict, image, phi, prefix=PREFIX, blocks=None):
    """The four backbone maps [B, C_i, H_i, W_i] in float64.  `blocks` (optional dict) receives every block output as 's<i>.b<j>'."""
    p = {k[len(prefix):]: v.detach().double() for k, v in state_dict.items() if k.startswith(prefix)}
    depths, dims = POOLFORMER[phi], WIDTHS[phi]
    x = F.conv2d(image.double(), p['patch_embed.proj.weight'], p['patch_embed.proj.bias'], stride=4, padding=2)
    outs = []
    for i in range(4):
        if i > 0:
            x = F.conv2d(x, p[f'network.{2 * i - 1}.proj.weight'], p[f'network.{2 * i - 1}.proj.bias'], stride=2, padding=1)
        assert x.shape[1] == dims[i]
        for j in range(depths[i]):
            b = f'network.{2 * i}.{j}.'
            n = group_norm1(x, p[b + 'norm1.weight'], p[b + 'norm1.bias'])
            x = x + p[b + 'layer_scale_1'].view(1, -1, 1, 1) * (F.avg_pool2d(n, 3, stride=1, padding=1, count_include_pad=False) - n)
            n = group_norm1(x, p[b + 'norm2.weight'], p[b + 'norm2.bias'])
            h = F.gelu(F.conv2d(n, p[b + 'mlp.fc1.weight'], p[b + 'mlp.fc1.bias']))
            x = x + p[b + 'layer_scale_2'].view(1, -1, 1, 1) * F.conv2d(h, p[b + 'mlp.fc2.weight'], p[b + 'mlp.fc2.bias'])
            if blocks is not None:
                blocks[f's{i}.b{j}'] = x
        outs.append(group_norm1(x, p[f'norm{2 * i}.weight'], p[f'norm{2 * i}.bias']))
    return outs
