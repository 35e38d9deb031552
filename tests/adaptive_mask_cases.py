"""Shared by tests/test_adaptive_mask_host.py and tests/test_gpu_adaptive_mask.py: the volumes and binary cases of the device
adaptive mask, NumPy restatements of its definition (the Gaussian passes, the histogram by edges, the composition with the
all-ties seed rule) and the margin checks that make "equal to the host's mask" a fair demand of a device filter that may
differ from SciPy's by rounding."""
import importlib
from pathlib import Path

import numpy as np

T = importlib.import_module("helicon_amd.true_fsc")

GOLDEN = Path(__file__).resolve().parent / "golden"

# (shape, sigma): the six cases on which the loop form below is SciPy 1.15.3's output bit for bit
GAUSS_CASES = (((20, 27, 33), 2.1), ((24, 24, 24), 0.787), ((5, 7, 3), 3.0), ((1, 1, 64), 1.3), ((40, 40, 40), 2.0997), ((3, 2, 9), 5.5))
FIXTURE_MODES = (dict(), dict(mask_fraction_thresh=0.3), dict(mask_thresh=0.5), dict(mask_mass=40.0))
N_SEEDS = 1000


def volume(shape, seed=0):
    return np.random.RandomState(seed).normal(size=shape)


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def bound(sigma, V):
    """3 (2 r + 3) 2^-53 max |V|: 2 r + 1 products and sums per pass with weights that sum to 1, three passes."""
    return 3.0 * (2 * radius(sigma) + 3) * 2.0**-53 * float(np.abs(V).max()) if sigma else 0.0


def fold(i, n):
    """scipy's reflect: d c b a | a b c d | d c b a, period 2 n."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def gaussian_numpy(V, sigma, taps=None):
    """The definition: passes z, y, x on float64; t = v[i] w[0], then for j = r ... 1: t += (v[i - j] + v[i + j]) w[j]."""
    w = T.gaussian_taps(sigma) if taps is None else taps
    r = len(w) - 1
    v = np.asarray(V, dtype=np.float64)
    for axis in (0, 1, 2):
        v = np.moveaxis(v, axis, -1)
        n = v.shape[-1]
        i = np.arange(n)
        t = v[..., i] * w[0]
        for j in range(r, 0, -1):
            t = t + (v[..., fold(i - j, n)] + v[..., fold(i + j, n)]) * w[j]
        v = np.moveaxis(t, -1, axis)
    return np.ascontiguousarray(v)


def counts_by_edges(x, edges):
    """Bin i holds edges[i] <= x < edges[i + 1]; the last bin is closed.  Every x lies in [edges[0], edges[-1]]."""
    idx = np.searchsorted(edges, x, side="right") - 1
    idx[idx == len(edges) - 1] = len(edges) - 2
    return np.bincount(idx, minlength=len(edges) - 1)


def low_pass(V, apix, cutoff_res):
    from scipy.ndimage import gaussian_filter

    V = np.asarray(V, dtype=np.float64)
    if cutoff_res > 2 * apix:
        return gaussian_filter(V, sigma=cutoff_res / (3.81 * apix)), cutoff_res / (3.81 * apix)
    return V.copy(), 0.0


def threshold(LP, apix, mask_fraction_thresh=0, mask_thresh=0, mask_mass=0):
    """(threshold, rank or None) in adaptive_mask's precedence; Otsu by the edges rule and otsu_from_counts."""
    if mask_fraction_thresh > 0:
        return mask_fraction_thresh * np.max(LP), None
    if mask_thresh and mask_thresh > 0:
        return mask_thresh, None
    if mask_mass > 0:
        k = min(int(mask_mass * 1e3 / (0.81 * apix**3)), LP.size - 1)
        return np.sort(LP.ravel())[::-1][k], k
    flat = LP.ravel()
    hmin, hmax = float(flat.min()), float(flat.max())
    counts = counts_by_edges(flat[flat != 0], np.linspace(hmin, hmax, 257))
    return T.otsu_from_counts(counts, hmin, hmax), None


def adaptive_mask_numpy(V, apix, cutoff_res, **kw):
    """The definition with the all-ties seed rule: (mask uint8, LP, threshold, v*, number of voxels >= v*)."""
    from scipy.ndimage import label

    LP, _ = low_pass(V, apix, cutoff_res)
    thresh, _ = threshold(LP, apix, **kw)
    v_star = np.partition(LP.ravel(), -N_SEEDS)[-N_SEEDS]
    above = LP > thresh
    labeled, _ = label(above, structure=np.ones((3, 3, 3), dtype=bool))
    seeds = np.unique(labeled[(LP >= v_star) & above])
    mask = np.isin(labeled, seeds[seeds > 0])
    if not mask.any():
        mask = above
    return mask.astype(np.uint8), LP, thresh, v_star, int((LP >= v_star).sum())


def check_margins(V, apix, cutoff_res, host_mask=None, **kw):
    """The conditions under which a filter within B = bound of SciPy's must give the host's mask.  Returns the figures."""
    LP, sigma = low_pass(V, apix, cutoff_res)
    B = bound(sigma, V)
    thresh, rank = threshold(LP, apix, **kw)
    flat = LP.ravel()
    fig = {"B": B, "threshold": float(thresh)}
    fig["to_threshold"] = float(np.abs(flat - thresh).min()) if rank is None else None
    desc = np.sort(flat)[::-1]
    if B > 0:
        if rank is None:
            assert fig["to_threshold"] > 2 * B, fig                      # no voxel within 2 B of the threshold
        if not any(kw.get(k, 0) for k in ("mask_fraction_thresh", "mask_thresh", "mask_mass")):
            edges = np.linspace(flat.min(), flat.max(), 257)[1:-1]
            nz = flat[flat != 0]
            near = np.searchsorted(edges, nz)
            gap = np.minimum(np.abs(nz - edges[np.clip(near, 0, 254)]), np.abs(nz - edges[np.clip(near - 1, 0, 254)]))
            fig["to_edge"] = float(gap.min())
            assert fig["to_edge"] > 2 * B, fig                           # no non-zero voxel within 2 B of an inner edge
        for name, k in (("rank", rank), ("seed", N_SEEDS - 1)):
            if k is None:
                continue
            gaps = [desc[k - 1] - desc[k] if k > 0 else np.inf, desc[k] - desc[k + 1] if k + 1 < len(desc) else np.inf]
            fig[f"{name}_gap"] = float(min(gaps))
            assert min(gaps) > 2 * B, fig                                # the neighbours of the rank are more than 2 B away
    n_ge = int((flat >= desc[N_SEEDS - 1]).sum())
    fig["n_ge"] = n_ge
    if n_ge != N_SEEDS:                                                   # ties at v*: the all-ties rule must give the host's mask
        assert host_mask is not None and np.array_equal(adaptive_mask_numpy(V, apix, cutoff_res, **kw)[0], np.asarray(host_mask) != 0), fig
    return fig


# ------------------------------------------------------------------------------------------
# the reference's recorded masks
# ------------------------------------------------------------------------------------------
def fixture_cases():
    """[(k, j, avg float64, apix, cutoff, mode, recorded mask uint8)] for the eight masks of g20_true_fsc.npz."""
    g = np.load(GOLDEN / "g20_true_fsc.npz")
    out = []
    for k in range(int(g["n_cases"][0])):
        n, _, cutoff, apix, _ = g[f"c{k}_par"]
        n = int(n)
        a, b = g[f"c{k}_a"].astype(np.float32), g[f"c{k}_b"].astype(np.float32)
        avg = (a.astype(np.float64) + b.astype(np.float64)) / 2
        for j, mode in enumerate(FIXTURE_MODES):
            want = np.unpackbits(g[f"c{k}_adaptive{j}"])[: n**3].reshape(n, n, n)
            out.append((k, j, avg, float(apix), float(cutoff), mode, want))
    return out


# ------------------------------------------------------------------------------------------
# synthetic volumes for the mask
# ------------------------------------------------------------------------------------------
def _gauss_blob(shape, centre, width, height):
    z, y, x = np.ogrid[: shape[0], : shape[1], : shape[2]]
    return height * np.exp(-((z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2) / (2.0 * width**2))


def blob_noise(shape, seed):
    c = tuple(s // 2 for s in shape)
    return _gauss_blob(shape, c, min(shape) / 6.0, 6.0) + np.random.RandomState(seed).normal(size=shape)


def bright_and_dim(shape=(40, 40, 40)):
    """A bright blob with more than 1000 voxels above the dim one's peak, and a distant dim blob: above a value threshold of
    0.5, without a seed."""
    return _gauss_blob(shape, (14, 14, 14), 7.0, 10.0) + _gauss_blob(shape, (33, 33, 33), 2.0, 1.2) + 0.01 * np.random.RandomState(5).normal(size=shape)


def two_blobs(shape=(40, 40, 40)):
    """Two separated blobs of nearly equal height: both hold some of the 1000 brightest voxels."""
    return _gauss_blob(shape, (11, 12, 12), 4.5, 8.0) + _gauss_blob(shape, (29, 28, 29), 4.5, 7.9) + 0.01 * np.random.RandomState(6).normal(size=shape)


def synthetic_cases():
    """[(name, V float64, apix, cutoff, mode)]"""
    cases = []
    for name, V in (("blob40", blob_noise((40, 40, 40), 11)), ("blob33x20x27", blob_noise((33, 20, 27), 12))):
        for tag, mode in (("otsu", dict()), ("fraction", dict(mask_fraction_thresh=0.25)), ("value", dict(mask_thresh=0.8)), ("mass", dict(mask_mass=2.0))):
            cases.append((f"{name}-{tag}", V, 1.0, 8.0, mode))
    cases.append(("bright+dim-value", bright_and_dim(), 1.0, 8.0, dict(mask_thresh=0.25)))
    cases.append(("two-blobs-fraction", two_blobs(), 1.0, 8.0, dict(mask_fraction_thresh=0.3)))
    cases.append(("above-the-maximum", blob_noise((40, 40, 40), 11), 1.0, 8.0, dict(mask_thresh=1e3)))
    return cases


# ------------------------------------------------------------------------------------------
# binary volumes for the labelling
# ------------------------------------------------------------------------------------------
def canonical(labels):
    """Labels renumbered 1 ... in the order of each label's first voxel; 0 stays."""
    flat = np.asarray(labels).ravel()
    vals, first = np.unique(flat, return_index=True)
    keep = vals != 0
    vals, first = vals[keep], first[keep]
    order = np.argsort(first)
    table = np.zeros(int(flat.max()) + 1 if flat.size else 1, dtype=np.int64)
    table[vals[order]] = np.arange(1, len(vals) + 1)
    return table[flat].reshape(np.shape(labels))


def scipy_labels(binary):
    from scipy.ndimage import label

    return label(np.asarray(binary) != 0, structure=np.ones((3, 3, 3), dtype=bool))


def serpentine(shape=(24, 24, 64)):
    """A one-voxel-wide path: x-runs on every second line of every second plane, joined at alternating ends."""
    nz, ny, nx = shape
    S = np.zeros(shape, np.uint8)
    turn = 0
    for z in range(0, nz, 2):
        ys = list(range(0, ny, 2))
        if (z // 2) % 2:
            ys.reverse()
        for k, y in enumerate(ys):
            S[z, y, :] = 1
            if k + 1 < len(ys):                                           # the link to the next line, at alternating ends
                S[z, (y + ys[k + 1]) // 2, nx - 1 if turn % 2 == 0 else 0] = 1
                turn += 1
        if z + 2 < nz:                                                    # the link to the next plane
            S[z + 1, ys[-1], nx - 1 if turn % 2 == 0 else 0] = 1
            turn += 1
    return S


def comb(shape=(6, 17, 130)):
    """Long x-runs on every second line, joined only at x = nx - 1: the roots must travel back along every run."""
    S = np.zeros(shape, np.uint8)
    S[::2, ::2, :] = 1
    S[:, :, -1] = 1
    return S


def helix(shape=(40, 21, 23)):
    S = np.zeros(shape, np.uint8)
    for k in range(shape[0] * 8):
        z = k / 8.0
        y = int(round(10 + 8 * np.sin(z * 0.7)))
        x = int(round(11 + 8 * np.cos(z * 0.7)))
        S[int(z), y, x] = 1
    return S


def label_cases():
    cases = []
    for shape in ((33, 20, 27), (70, 66, 130)):
        for p in (0.08, 0.12, 0.2, 0.5):
            rng = np.random.RandomState(int(p * 100) + shape[0])
            cases.append((f"bernoulli-{p}-{'x'.join(map(str, shape))}", (rng.uniform(size=shape) < p).astype(np.uint8)))
    corner = np.zeros((4, 5, 6), np.uint8)
    corner[1, 1, 1] = corner[2, 2, 2] = 1
    edge = np.zeros((4, 5, 6), np.uint8)
    edge[1, 1, 1] = edge[1, 2, 2] = 1
    z, y, x = np.ogrid[:9, :10, :11]
    checker = ((x + y + z) % 2 == 0).astype(np.uint8)
    single = np.zeros((5, 6, 7), np.uint8)
    single[2, 3, 4] = 1
    line = np.ones((1, 1, 130), np.uint8)
    line[0, 0, [0, 5, 63, 64, 100, 128]] = 0
    long = (np.random.RandomState(5).uniform(size=(8, 8, 1024)) < 0.3).astype(np.uint8)
    long[2, 3, 100:900] = 1
    tall = (np.random.RandomState(6).uniform(size=(1024, 3, 2)) < 0.4).astype(np.uint8)
    cases += [("corner", corner), ("edge", edge), ("checkerboard", checker), ("serpentine", serpentine()), ("comb", comb()), ("helix", helix()),
              ("full", np.ones((7, 9, 70), np.uint8)), ("empty", np.zeros((7, 9, 11), np.uint8)), ("single", single), ("1x1x130", line),
              ("8x8x1024", long), ("1024x3x2", tall)]
    return cases
