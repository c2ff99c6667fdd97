"""The multigrid pressure solve of vpt_scene_fluid_step_solver (include/vpt.h) restated in numpy, vectorised, in float64 - or in the dtype
asked for: the float32 run of this file against its float64 run is the yardstick tests/test_fluid_mg_host.py holds the host mirror to.
Fields are (d, h, w) arrays as in fluid_exact.py, whose neighbour shifts this file uses; nothing here shares a line with
csrc/vpt_fluid_rule.h."""
import numpy as np

import fluid_exact as ex


def level_shapes(shape):
    """(d, h, w) of every level, finest first: halves rounded up until every axis is <= 8"""
    out = [tuple(shape)]
    while max(out[-1]) > 8:
        out.append(tuple((n + 1) // 2 for n in out[-1]))
    return out


class Level:
    """the operator of level l: wgt[c] the face weight along component c at every node, D its diagonal, s its factor"""

    def __init__(self, shape, shape0, l, open_faces, dtype):
        cover = [np.minimum(2 ** l, n0 - np.arange(n) * 2 ** l).astype(dtype) for n, n0 in zip(shape, shape0)]   # along z, y, x
        cz, cy, cx = cover[0][:, None, None], cover[1][None, :, None], cover[2][None, None, :]
        one = np.ones(shape, dtype)
        self.wgt = [cy * cz * one, cx * cz * one, cx * cy * one]
        self.D = np.zeros(shape, dtype)
        for c in range(3):
            for side in (0, 1):   # a direction counts where its neighbour is inside, and on the face where the face is open
                counts = ex.shifted(one, c, side, 1.0 if ex.is_open(open_faces, c, side) else 0.0)
                self.D = self.D + self.wgt[c] * counts
        self.s = dtype(1.5) ** l
        self.open_faces, self.dtype = open_faces, dtype
        at = np.indices(shape).sum(axis=0)
        self.colour = [(at & 1) == 0, (at & 1) == 1]

    def S(self, p):
        return sum(self.wgt[c] * ex.shifted(p, c, side, 0.0) for c in range(3) for side in (0, 1))

    def half_sweep(self, p, b, colour):
        with np.errstate(divide="ignore", invalid="ignore"):
            new = (self.S(p) + self.s * b) / self.D
        return np.where(self.colour[colour] & (self.D != 0), new, p)

    def sweeps(self, p, b, count, first):
        for _ in range(count):
            p = self.half_sweep(self.half_sweep(p, b, first), b, first ^ 1)
        return p

    def residual(self, p, b):
        return b - (self.D * p - self.S(p)) / self.s


def restrict(r):
    d, h, w = ((n + 1) // 2 for n in r.shape)
    pad = np.pad(r, [(0, 2 * n - m) for n, m in zip((d, h, w), r.shape)])
    return pad.reshape(d, 2, h, 2, w, 2).sum(axis=(1, 3, 5))


def prolong(coarse, shape):
    fine = coarse.repeat(2, axis=0).repeat(2, axis=1).repeat(2, axis=2)
    return fine[:shape[0], :shape[1], :shape[2]]


def cycle(levels, l, p, b, smooth, coarse_sweeps):
    g = levels[l]
    if l == len(levels) - 1:
        return g.sweeps(p, b, coarse_sweeps, 0)
    p = g.sweeps(p, b, smooth, 0)
    down = restrict(g.residual(p, b))
    p = p + prolong(cycle(levels, l + 1, np.zeros_like(down), down, smooth, coarse_sweeps), p.shape)
    return g.sweeps(p, b, smooth, 1)


def pressure(div, open_faces, cycles, smooth, coarse_sweeps, dtype=np.float64):
    """p after `cycles` V-cycles from 0 for the divergence `div`"""
    shapes = level_shapes(div.shape)
    levels = [Level(shape, shapes[0], l, open_faces, dtype) for l, shape in enumerate(shapes)]
    p, b = np.zeros(div.shape, dtype), -div.astype(dtype)
    for _ in range(cycles):
        p = cycle(levels, 0, p, b, smooth, coarse_sweeps)
    return p


def residual_norm(p, div, open_faces):
    """the L2 norm of the mean-free part of -d - (D p - S) at level 0, in float64"""
    r = Level(div.shape, div.shape, 0, open_faces, np.float64).residual(p.astype(np.float64), -div.astype(np.float64))
    return float(np.linalg.norm(r - r.mean()))
