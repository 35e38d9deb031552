"""Shared by tests/test_soft_mask_host.py and tests/test_gpu_soft_mask.py: the supports and widths of the device soft-mask
tests, a NumPy composition of the definition (integer distance transform, zoom's tap tables, the edge rule) and a stand-in for
the resident context that builds its soft masks on the host."""
import importlib

import numpy as np

import true_fsc_oracle as TO

T = importlib.import_module("helicon_amd.true_fsc")

# box, centre, r^2 of (z - cz)^2 + 1.4 (y - cy)^2 + (x - cx)^2 < r^2
BOXES = (((24, 24, 24), (12, 11, 13), 30), ((26, 26, 26), (13, 12, 14), 30), ((44, 44, 44), (22, 20, 23), 90), ((20, 27, 33), (10, 13, 17), 25))
WIDTHS = (2.5, 9.3, 13.7)       # steps 1, 2, 3
TIE = 1e-9
INF = 1 << 28


def ellipsoid(shape, centre, r2):
    z, y, x = np.ogrid[: shape[0], : shape[1], : shape[2]]
    return ((z - centre[0]) ** 2 + 1.4 * (y - centre[1]) ** 2 + (x - centre[2]) ** 2 < r2).astype(np.uint8)


def cube_support(n):
    """The ellipsoid of the n^3 box (24, 26, 44)."""
    for shape, centre, r2 in BOXES:
        if shape == (n, n, n):
            return ellipsoid(shape, centre, r2)
    raise KeyError(n)


def edt_sq(inside):
    """The exact squared Euclidean distance to the nearest True voxel, int64: min-plus envelopes along x, y, z."""
    g = np.where(np.asarray(inside, dtype=bool), 0, INF).astype(np.int64)
    for axis in (2, 1, 0):
        g = np.moveaxis(g, axis, -1)
        m = g.shape[-1]
        i = np.arange(m)
        g = np.minimum((g[..., None, :] + (i[:, None] - i[None, :]) ** 2).min(axis=-1), INF)
        g = np.moveaxis(g, -1, axis)
    return g


def zoomed(dist_ds, shape, taps=None, outside_rule=True):
    """zoom(order=1) of a 3-D array to `shape` from the per-axis tap tables: eight taps, z, y, x."""
    taps = taps or T.zoom_taps
    tz, ty, tx = (taps(n, m) for n, m in zip(shape, dist_ds.shape))
    out = np.zeros(shape, dtype=np.float64)
    for p in (0, 1):
        for q in (0, 1):
            for r in (0, 1):
                v = dist_ds[np.ix_(tz[p], ty[q], tx[r])]
                out += v * tz[2 + p][:, None, None] * ty[2 + q][None, :, None] * tx[2 + r][None, None, :]
    if outside_rule:
        out[tz[4], :, :] = 0.0
        out[:, ty[4], :] = 0.0
        out[:, :, tx[4]] = 0.0
    return out


def distance(mask, width, taps=None):
    step = max(1, int(width / 4))
    ds = np.asarray(mask)[::step, ::step, ::step] != 0
    return zoomed(step * np.sqrt(edt_sq(ds).astype(np.float64)), np.asarray(mask).shape, taps)


def soft_mask_numpy(mask, width, taps=None):
    """(soft, dist): the definition, in float64."""
    mask = np.asarray(mask)
    dist = distance(mask, width, taps)
    outside = mask == 0
    soft = np.ones(mask.shape, dtype=np.float64)
    edge = outside & (dist > 0) & (dist <= width)
    soft[edge] = (np.cos(dist[edge] / width * np.pi / 2) + 1) / 2
    soft[outside & (dist > width)] = 0.0
    return soft, dist


def tie_margin(mask, width):
    """min |dist - width| over the outside voxels: the distance of the case from a tie."""
    _, dist = soft_mask_numpy(mask, width)
    return float(np.abs(dist[np.asarray(mask) == 0] - width).min())


class HostSoftOracle(TO.OracleTrueFSC):
    """OracleTrueFSC with TrueFSC's soft-mask methods, the masks built by the host's soft_mask; counts its calls."""

    log = []

    def set_support(self, support1, support2=None):
        type(self).log.append(("set_support", support2 is not None))
        self._sup = [np.asarray(support1) != 0] + ([] if support2 is None else [np.asarray(support2) != 0])

    def soft_mask(self, width, which=0):
        type(self).log.append(("soft_mask", float(width), which))
        return T.soft_mask(self._sup[which if len(self._sup) == 2 else 0], width).astype(np.float32)

    def soft_masked(self, width, per_shell=False):
        type(self).log.append(("soft_masked", float(width), bool(per_shell)))
        m = [T.soft_mask(s, width).astype(np.float32) for s in self._sup]
        return super().masked(m[0], m[-1] if len(m) == 2 else None, per_shell=per_shell)

    def masked(self, mask1, mask2=None, per_shell=False):
        type(self).log.append(("masked",))
        return super().masked(mask1, mask2, per_shell=per_shell)
