"""Clouds for tests/test_pn2_geometry.py: the inputs at which the index selection of k_pn2.h meets TIES, which the Gaussian clouds of `synth.make_inputs` (512 distinct points)
never produce, and the counters that prove — from the oracle alone — that a cloud holds the ties it was built for.

  * `resampled`: a frame's few radar returns drawn N times WITH replacement and column-normalised, as the reference's loader builds a cloud (utils/dataloader.py:137,
    achelous.py:240): a few dozen distinct points among N, so most farthest-point picks are made among all-zero distances, every ball overflows and most 3-NN choices are ties
    between coincident centroids;
  * `lattice`: coordinates that are integer multiples of 2^-5 in a small box, so every squared distance is an integer multiple of 2^-10 and exact in fp32: with a squared
    radius of 2 * 2^-10 or 3 * 2^-10 points sit exactly ON the `<=` boundary of a ball, and farthest-point ties occur at equal NON-ZERO distances."""
import numpy as np
import torch

from achelous_amd.synth import make_inputs
from oracle import pointnet2_oracle as po

LATTICE_STEP = 2.0 ** -5


def resampled(xp, distinct, seed):
    """xp [B, C, N] (the point tensor of `make_inputs`) -> [B, C, N]: per frame `distinct` of its points are kept, N are drawn from them with replacement, and every
    feature column is L2-normalised over the N points again, as `make_inputs` does."""
    g = torch.Generator().manual_seed(int(seed))
    B, C, N = xp.shape
    rows = torch.empty(B, N, C, dtype=xp.dtype)
    for b in range(B):
        keep = torch.randperm(N, generator=g)[:distinct]
        draw = keep[torch.randint(0, len(keep), (N,), generator=g)]
        rows[b] = xp[b].t()[draw]
    rows = rows / rows.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return rows.transpose(1, 2).contiguous()


def cloud(batch, n, distinct, seed, channels=3):
    """[batch, n, channels] rows of `batch` different clouds: `make_inputs` points, `resampled` to `distinct` points per cloud (None: left as drawn)."""
    xp = make_inputs(batch, seed, resolution=32, num_points=n, pc_channels=channels, radar_cells=4)[2]
    if distinct is not None:
        xp = resampled(xp, distinct, seed)
    return xp.transpose(1, 2).contiguous()


def lattice(n, seed, side=6):
    """[n, 3] float32: n points on the side^3 sites of a lattice of step 2^-5 centred on the origin (n > side^3 / 2: coincident points too).  NOT normalised: the
    coordinates stay exact."""
    g = torch.Generator().manual_seed(int(seed))
    return ((torch.randint(0, side, (n, 3), generator=g) - side // 2).float() * LATTICE_STEP).contiguous()


def lattice_clouds(batch, n, seed, side=6):
    return torch.stack([lattice(n, seed + 101 * b, side) for b in range(batch)])


def lattice_radius(k):
    """The radius whose fp32 square is exactly k * 2^-10 (k = 2, 3: the lattice offsets (1, 1, 0) and (1, 1, 1) lie ON the boundary)."""
    r = float(np.sqrt(k * 2.0 ** -10))
    assert np.float32(r * r) == np.float32(k * 2.0 ** -10)
    return r


# ---------------------------------------------------------------------------------------------------- what a cloud contains, by the oracle's own arithmetic
def fps_tie_picks(xyz, npoint):
    """-> (picks made among several holders of the maximum, those of them at an all-zero maximum), over the npoint - 1 arg-max selections of `po.farthest_point_sample`."""
    xyz = np.asarray(xyz, np.float32)
    dist = np.full(len(xyz), 1e10, np.float32)
    far, ties, zeros = 0, 0, 0
    for _ in range(npoint - 1):
        dist = np.minimum(dist, po.sqdist(xyz, xyz[far:far + 1])[:, 0])
        m = dist.max()
        if int((dist == m).sum()) > 1:
            ties += 1
            zeros += int(m == 0)
        far = int(np.argmax(dist))
    return ties, zeros


def ball_fill(radius, nsample, xyz, new_xyz):
    """-> (balls with fewer than nsample members, balls with more, balls with a member exactly on the boundary d == r^2)."""
    d = po.sqdist(np.asarray(new_xyz, np.float32), np.asarray(xyz, np.float32))
    r2 = np.float32(radius * radius)
    members = (d <= r2).sum(1)
    return int((members < nsample).sum()), int((members > nsample).sum()), int((d == r2).any(1).sum())


def interp_tied_rows(xyz1, xyz2):
    """-> dense points whose 3rd and 4th nearest sparse points are at equal distance (the third neighbour is decided by the tie rule)."""
    d = np.sort(po.sqdist(np.asarray(xyz1, np.float32), np.asarray(xyz2, np.float32)), axis=1)
    return int((d[:, 2] == d[:, 3]).sum()) if d.shape[1] > 3 else 0
