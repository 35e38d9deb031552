"""The true-FSC context (hh_tfsc_*; helicon_amd/csrc/true_fsc.inc) on every even side around its tiles: the sides, the inputs,
the cutoff rule, the comparison with the float64 oracle (``compare``), a float32 model of the device's pipeline that can be
given one fault at a time (``ModelTrueFSC``), and the device generator restated on the host (``philox_angles``).  No GPU
dependency and no import of the package under test: NumPy, SciPy, tests/fsc_oracle.py and tests/true_fsc_oracle.py only.

Why: k_tfsc_xpass, k_tfsc_c2r and the inverse z / y passes (k_circ_gemm<false>) tile rows = n^2 by 64 and the columns by 64 in
two 32-wide sub-tiles; the c2r sum runs over ncol = n / 2 + 1 in slices of FC_K = 32 and the inverse operators over 2 n.
For even n, n^2 mod 64 is 0, 4, 16 or 36:

    n mod 16    n^2 mod 64    the last tile of 64 rows
    0, 8        0             whole
    2, 14       4             lower 32-row sub-tile: 4 rows (h = 0, i < 4); the upper one inactive
    4, 12       16            lower sub-tile: 16 rows; the upper one inactive
    6, 10       36            lower sub-tile whole; the upper one: 4 rows

(n = 16 a + r: n^2 = r^2 + 32 a r mod 64, and 32 a r = 0 mod 64 for even r.)  The rows a wrong guard loses are kz = n - 1: low
frequencies, every curve moves.

``SIDES``: every even side 8 ... 72, plus 126 and 130: all four residues, ncol = 5 ... 37 across the 32-column sub-tile and
the FC_K slice, ncol = 64 and 66 (65 is side 128, tests/test_gpu_true_fsc.py), n = 62 / 64 / 66 / 70 around k_circ_gemm's
64-row operator tile, every even 2 n mod 32, both classes of n mod 4.

Cutoff: ``cutoff(n) = APIX n / q(n)``, q = n / 4 + 1/2 when 4 divides n and n / 4 + 1/4 otherwise, so that
(apix / cutoff)^2 n^2 = q^2 is never an integer (n = 4 j: j^2 + j + 1/4; n = 4 j + 2: q = j + 3/4, j^2 + 3/2 j + 9/16, fraction 9/16 or 1/16) and no
bin is a tie; (n / 4 + 1/2)^2 = (j + 1)^2 would be one for n = 4 j + 2.

Bounds (those of tests/test_gpu_true_fsc.py, none measured): 3e-7 for curves that see forward passes only, 9e-7 for curves
that see forward, inverse and forward passes, 2^-22 for |F'| against |F|, 8 x the distance of SciPy's own float32 transform
from float64 on the same data for the randomised map (irfftn) and for the stored spectrum (rfftn), bit equality for the
frequency column and for the bins below the cutoff.  Generator: 2^-23 |F| per component (one float32 rounding, 2^-24, plus
the float64 sincos and square root).
"""
from __future__ import annotations

import numpy as np

import fsc_oracle as O
import true_fsc_oracle as TO

SIDES = tuple(range(8, 73, 2)) + (126, 130)
GENERATOR_SIDES = (10, 14, 30, 66, 130)
GENERATOR_SEED = 0x1234567887654321
FAULT_SIDES = (10, 14, 66)

APIX = 2.0
TOL_FSC_3D = 3e-7
TOL_ROUND_TRIP = 9e-7
TOL_AMP = 2.0**-22
TOL_ANGLE = 2.0**-23
TRANSFORM_FACTOR = 8
FLOOR = 1e-4


def q_of(n):
    return n / 4 + (0.5 if n % 4 == 0 else 0.25)


def cutoff(n):
    return APIX * n / q_of(n)


def inputs(n):
    """(map1, map2, (angles1, angles2)): tests/test_gpu_true_fsc.py's."""
    a, b = O.make_map_pair(n, 3000 + n, dc="auto")
    rng = np.random.RandomState(n)
    shape = (n, n, n // 2 + 1)
    return a, b, (rng.uniform(0, 2 * np.pi, size=shape), rng.uniform(0, 2 * np.pi, size=shape))


def masks(n):
    return TO.sphere_mask(n, 0.3 * n, 4.0), TO.sphere_mask(n, 0.35 * n, 3.0)


class _Oracle(TO.OracleTrueFSC):
    """The oracle with its masked sums kept: ``preconditions`` and ``compare`` ask for the same ones."""

    def masked_sums(self, masks1, masks2=None, per_shell=False):
        memo = self.__dict__.setdefault("_memo", {})
        key = (np.asarray(masks1).tobytes(), None if masks2 is None else np.asarray(masks2).tobytes(), bool(per_shell))
        key = tuple(hash(k) for k in key)
        if key not in memo:
            memo[key] = super().masked_sums(masks1, masks2, per_shell)
        return memo[key]


def oracle(n, phases=None):
    a, b, u = inputs(n)
    return _Oracle(a, b, APIX, cutoff(n), phases=u if phases is None else phases)


def residues(n):
    """What of the kernels' tiling a side reaches."""
    ncol = n // 2 + 1
    return dict(rows_mod_64=n * n % 64, n_mod_4=n % 4, ncol=ncol, ncol_side_of_32=int(np.sign(ncol - 32)),
                ncol_side_of_64=int(np.sign(ncol - 64)), n_side_of_64=int(np.sign(n - 64)), ka_mod_32=2 * n % 32)


# ------------------------------------------------------------------------------------------
# preconditions of the comparison, from the oracle alone
# ------------------------------------------------------------------------------------------
def preconditions(ora, n, masked=None):
    """The cutoff makes no tie and the integer rule selects the reference expression's bins; the smallest floor ratio of every
    pair whose curve is compared.  ``masked``: {per_shell: ora.masked_sums(mask[None], None, per_shell)[0]} if already there."""
    q = q_of(n)
    sel = TO.m_half(n) >= ora.m_cut
    m1 = masks(n)[0]
    out = dict(q2_fraction=float(q * q - np.floor(q * q)), m_cut_is_ceil=ora.m_cut == int(np.ceil(q * q)),
               same_bins=bool(np.array_equal(sel, TO.reference_cutoff_mask(n, APIX, cutoff(n)))),
               cutoff_index_is_n_over_4=ora.cutoff_index == n // 4, randomised=int(sel.sum()),
               floor_unmasked=O.floor_ratio(ora.sums[0]), floor_randomised=O.floor_ratio(ora.sums[1]))
    for per_shell in (False, True):
        s = masked[per_shell] if masked is not None else ora.masked_sums(m1[None], None, per_shell)[0]
        key = "full" if per_shell else "half"
        out[f"floor_masked_{key}"] = O.floor_ratio(s[0])
        out[f"floor_randomised_masked_{key}"] = O.floor_ratio(s[1])
    return out


def preconditions_hold(p):
    floors = [v for k, v in p.items() if k.startswith("floor_")]
    return (0 < p["q2_fraction"] < 1 and p["m_cut_is_ceil"] and p["same_bins"] and p["cutoff_index_is_n_over_4"]
            and p["randomised"] > 0 and len(floors) == 6 and min(floors) >= FLOOR)


# ------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------
def _err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


def _bits_differ(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return 1.0
    return float(np.count_nonzero(x.view(np.uint8) != y.view(np.uint8)) != 0)


def sequential_dc(src32, slice_terms=32):
    """The DC bin as the device's three passes give it, in float32: one sequential sum along z and one along y (the MFMA's
    multiply-add chain of k_circ_gemm; every cosine is 1), then along x a chain per slice of ``slice_terms`` = FC_K terms and
    the slices added in order (fc_pair_product).  ``slice_terms=None``: one chain along x too."""
    p = np.zeros(src32.shape[1:], np.float32)
    for plane in src32:
        p = p + plane
    q = np.zeros(src32.shape[2], np.float32)
    for row in p:
        q = q + row
    total = np.float32(0)
    step = len(q) if slice_terms is None else slice_terms
    for k0 in range(0, len(q), step):
        r = np.float32(0)
        for v in q[k0: k0 + step]:
            r = np.float32(r + v)
        total = np.float32(total + r)
    return float(total)


def compare(dev, ora, n, plain=None, notes=None):
    """{figure: (value, bound)} of anything with TrueFSC's interface against the float64 oracle of the same inputs; a figure
    holds when value <= bound.  ``plain``: the two half spectra of the same pipeline with nothing substituted (the device's:
    a context with m_cut above every bin); default ``dev.plain``.  ``notes``: a dict that receives, per stored spectrum, the bin
    of the largest distance from float64, SciPy's own distance, and the distances of ``sequential_dc`` at the DC bin (the
    device's order, and one chain along x)."""
    from scipy.fft import irfftn, rfftn

    figs = {}

    def put(name, value, bound):
        figs[name] = (float(value), float(bound))

    plain = dev.plain if plain is None else plain
    sel = TO.m_half(n) >= ora.m_cut
    mask, mask2 = masks(n)
    put("cutoff", abs(dev.m_cut - ora.m_cut) + abs(dev.cutoff_index - ora.cutoff_index) + (dev.cutoff_res != ora.cutoff_res), 0)
    # the stored spectra and the randomised maps
    for which, (F, src, want) in enumerate(((ora.F1r, ora.a, ora.ar), (ora.F2r, ora.b, ora.br))):
        spec, P = dev.randomized_map(which, return_fft=True), plain[which]
        ok = spec.dtype == np.complex64 and spec.shape == (n, n, n // 2 + 1) == P.shape
        put(f"spec{which}_form", not ok, 0)
        if not ok:
            continue
        put(f"spec{which}_untouched_bits", _bits_differ(spec[~sel], P[~sel]), 0)
        amp, amp0 = np.abs(spec.astype(np.complex128)), np.abs(P.astype(np.complex128))
        put(f"spec{which}_amp_rel", (np.abs(amp - amp0)[sel] / amp0[sel].clip(1e-30)).max(), TOL_AMP)
        f_max = np.abs(F).max()
        src32 = src.astype(np.float32)
        dist = np.abs(rfftn(src32) - rfftn(src)).max() / f_max
        d_spec = np.abs(spec - F)
        put(f"spec{which}_vs_f64", d_spec.max() / f_max, TRANSFORM_FACTOR * dist)
        if notes is not None:
            notes[f"spec{which}_worst_bin"] = "(%d,%d,%d)" % np.unravel_index(int(d_spec.argmax()), d_spec.shape)
            notes[f"spec{which}_scipy_f32_dist"] = float(dist)
            notes[f"spec{which}_host_chain_dc"] = abs(sequential_dc(src32) - float(src.sum())) / f_max
            notes[f"spec{which}_host_one_chain_dc"] = abs(sequential_dc(src32, None) - float(src.sum())) / f_max
        got = dev.randomized_map(which)
        F32 = F.astype(np.complex64)
        w_max = np.abs(want).max()
        dist = np.abs(irfftn(F32) - TO.irfftn(F32)).max() / w_max
        put(f"map{which}_form", not (got.dtype == np.float32 and got.shape == want.shape), 0)
        put(f"map{which}_vs_f64", np.abs(got - want).max() / w_max, TRANSFORM_FACTOR * dist)
    # curves
    put("unmasked_saxis_bits", _bits_differ(dev.unmasked[:, 0], ora.unmasked[:, 0]), 0)
    put("unmasked", _err(dev.unmasked[:, 1], ora.unmasked[:, 1]), TOL_FSC_3D)
    put("randomised_unmasked_saxis_bits", _bits_differ(dev.randomized_unmasked[:, 0], ora.randomized_unmasked[:, 0]), 0)
    put("randomised_unmasked", _err(dev.randomized_unmasked[:, 1], ora.randomized_unmasked[:, 1]), TOL_FSC_3D)
    for per_shell in (False, True):
        key = "full" if per_shell else "half"
        t, nz = dev.masked(mask, per_shell=per_shell)
        wt, wn = ora.masked(mask, per_shell=per_shell)
        if not per_shell:
            put("masked_half_saxis_bits", _bits_differ(t[:, 0], wt[:, 0]) + _bits_differ(nz[:, 0], wn[:, 0]), 0)
            t, nz, wt, wn = t[:, 1], nz[:, 1], wt[:, 1], wn[:, 1]
        put(f"masked_{key}_fsc_t", _err(t, wt), TOL_FSC_3D)
        put(f"masked_{key}_fsc_n", _err(nz, wn), TOL_ROUND_TRIP)
        put(f"masked_{key}_numerator", _err(t - nz, wt - wn), TOL_ROUND_TRIP)
    t, nz = dev.masked(mask)
    put("true_fsc_is_corrected", _bits_differ(dev.true_fsc(mask)[:, 1], TO.corrected(t[:, 1], nz[:, 1], dev.cutoff_index)), 0)
    t, nz = dev.masked(mask, mask2)
    wt, wn = ora.masked(mask, mask2)
    put("two_masks_saxis_bits", _bits_differ(t[:, 0], wt[:, 0]), 0)
    put("two_masks_fsc_t", _err(t[:, 1], wt[:, 1]), TOL_FSC_3D)
    put("two_masks_fsc_n", _err(nz[:, 1], wn[:, 1]), TOL_ROUND_TRIP)
    return figs


def exceeded(figs):
    """The figures beyond their bound (NaN counts)."""
    return [k for k, (v, b) in figs.items() if not v <= b]


def figure_line(figs):
    return " ".join(f"{k}={v:.3e}/{b:.3e}" for k, (v, b) in figs.items() if b > 0)


# ------------------------------------------------------------------------------------------
# the device generator on the host
# ------------------------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 from its definition (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3; SC'11): ten
    rounds of (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key raised by the
    Weyl constants after each.  ``counter``: four, ``key``: two arrays (or integers) of 32-bit words; returns the four output
    words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & _LOW for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _LOW for v in key]
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                     # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> _32) ^ c[1] ^ k[0], p1 & _LOW, (p0 >> _32) ^ c[3] ^ k[1], p0 & _LOW]
        k = [(k[0] + _W0) & _LOW, (k[1] + _W1) & _LOW]
    return c


def philox_angles(n, seed):
    """(angles of map 1, of map 2), [n, n, n // 2 + 1] float64: tf_philox's draw of every bin.  Counter (bin lo, bin hi, map, 0),
    bin = (kz n + ky) ncol + kx; key (seed lo, seed hi); angle (first output word + 1/2) 2 pi / 2^32."""
    ncol = n // 2 + 1
    bins = np.arange(n * n * ncol, dtype=np.uint64)
    seed = int(seed) & (2**64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    zero = np.zeros_like(bins)
    out = []
    for which in (0, 1):
        word = philox4x32_10((bins & _LOW, bins >> _32, zero + np.uint64(which), zero), key)[0]
        out.append(((word.astype(np.float64) + 0.5) * (2 * np.pi / 4294967296.0)).reshape(n, n, ncol))
    return tuple(out)


def generator_figures(spec, plain, theta, sel):
    """(Re, Im): max over the substituted bins of |component - a component(e^{i theta})| / a, a the float64 modulus of the
    pipeline's own plain bin (a bin of modulus 0 must be 0)."""
    a = np.abs(plain.astype(np.complex128))[sel]
    want = a * np.exp(1j * theta[sel])
    got = spec.astype(np.complex128)[sel]
    scale = np.where(a > 0, a, 1e-300)
    return float((np.abs(got.real - want.real) / scale).max()), float((np.abs(got.imag - want.imag) / scale).max())


# ------------------------------------------------------------------------------------------
# a float32 model of the device's pipeline, with one fault at a time
# ------------------------------------------------------------------------------------------
FAULTS = {
    "spec_last_rows": "the last 4 of the n^2 rows of the stored half spectrum are 0",
    "map_last_rows": "the last 4 of the n^2 rows of the randomised maps are 0",
    "sums_last_rows": "the last 4 of the n^2 rows do not reach the two curves' sums",
    "column_32": "column kx = 32 of the stored half spectrum is 0 (sides with ncol > 32)",
    "ky_rows_swapped": "rows ky = 1 and ky = 2 of the stored half spectrum change places",
    "c2r_nyquist_weight_2": "the c2r sum gives column kx = n / 2 the weight 2",
    "c2r_sine_rows_live": "the c2r sine table's rows k = 0 and k = n / 2 are not 0",
    "full_sums_nyquist_weight_2": "the full-spectrum sums give column kx = n / 2 the weight 2",
    "angles_of_map_2_for_map_1": "map 1 is substituted with map 2's angles",
    "m_cut_plus_1": "the kernel substitutes from m_cut + 1 on",
    "m_cut_minus_1": "the kernel substitutes from m_cut - 1 on",
}


def weighted_half_sums(a, b, n, nyquist_weight=1.0):
    """The full-spectrum shell sums of two real maps from the half spectrum: weight 1 on kx = 0 and kx = n / 2, 2 elsewhere
    (k_fc_xpass's `weighted` form)."""
    F1, F2 = np.fft.rfftn(np.asarray(a, dtype=np.float64)), np.fft.rfftn(np.asarray(b, dtype=np.float64))
    w = np.full(n // 2 + 1, 2.0)
    w[0], w[n // 2] = 1.0, nyquist_weight
    s = O.shell_3d_half(n).ravel()
    W = np.broadcast_to(w, F1.shape)
    return np.stack([np.bincount(s, weights=(W * np.real(F1 * np.conj(F2))).ravel(), minlength=n // 2 + 1),
                     np.bincount(s, weights=(W * np.abs(F1) ** 2).ravel(), minlength=n // 2 + 1),
                     np.bincount(s, weights=(W * np.abs(F2) ** 2).ravel(), minlength=n // 2 + 1)], axis=1)


def c2r_tables(n, fault=None):
    """(cw, sw), [ncol, n] float64: y[x] = sum_k Re G_k cw[k, x] + Im G_k sw[k, x], tf_c2r_table's: w_k cos / n and -w_k sin / n
    with w = 1 on k = 0 and k = n / 2 and 2 elsewhere, the sine rows of those two k exactly 0.

    Fault c2r_sine_rows_live: sin(2 pi k x / n) IS 0 on those rows (float64 gives 1.2e-16 x at most), so leaving them to the
    formula moves nothing a float32 map can show.  What the zero rows stand for is that Im G_0 and Im G_{n/2}, which are not 0
    once the spectrum is no longer Hermitian-consistent, never reach the map; the fault lets them: the two rows hold their
    neighbours' (k = 1, k = n / 2 - 1)."""
    hn = n // 2
    k, x = np.arange(hn + 1)[:, None], np.arange(n)[None, :]
    w = np.full((hn + 1, 1), 2.0)
    w[0] = w[hn] = 1.0
    if fault == "c2r_nyquist_weight_2":
        w[hn] = 2.0
    arg = 2 * np.pi * ((k * x) % n) / n
    cw, sw = w * np.cos(arg) / n, -w * np.sin(arg) / n
    sw[0] = sw[hn] = 0.0
    if fault == "c2r_sine_rows_live":
        sw[0], sw[hn] = sw[1], sw[hn - 1]
    return cw, sw


class ModelTrueFSC:
    """TrueFSC's interface on the host, with the device's roundings: the forward transform in float64 rounded to float32 bins,
    the substitution |F| e^{i theta} from those bins rounded once more, the shell sums of the bins as stored, the inverse
    transform of the stored spectrum (complex passes along z and y, then the c2r tables) rounded to float32 maps, masked
    sums from the float32 maps.  ``fault``: one of ``FAULTS``, applied where the kernel would make it; what follows that
    stage sees it."""

    def __init__(self, map1, map2, apix, cutoff_res, *, phases, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault
        self.a, self.b = np.asarray(map1, dtype=np.float32), np.asarray(map2, dtype=np.float32)
        n = self.n = self.a.shape[0]
        ncol = n // 2 + 1
        self.apix, self.cutoff_res = float(apix), float(cutoff_res)
        self.cutoff_index = int(n * apix / cutoff_res)
        self.m_cut = int(np.ceil((apix / cutoff_res) ** 2 * n * n - 1e-9))
        used = self.m_cut + {"m_cut_plus_1": 1, "m_cut_minus_1": -1}.get(fault, 0)
        self.sel_used = TO.m_half(n) >= used
        th = [np.asarray(p, dtype=np.float64) for p in phases]
        if fault == "angles_of_map_2_for_map_1":
            th[0] = th[1]
        bins = [np.fft.rfftn(m.astype(np.float64)).astype(np.complex64) for m in (self.a, self.b)]
        subst = []
        for F, t in zip(bins, th):
            S = F.copy()
            amp = np.abs(F.astype(np.complex128))
            S[self.sel_used] = (amp * np.exp(1j * t))[self.sel_used].astype(np.complex64)
            subst.append(S)
        keep = np.ones((n * n, ncol), dtype=bool)
        if fault == "sums_last_rows":
            keep[-4:] = False
        keep = keep.reshape(n, n, ncol)
        both = [[F.astype(np.complex128) * keep for F in pair] for pair in (bins, subst)]
        self.sums = np.stack([TO.sums_of_spectra(*pair) for pair in both])
        self.unmasked = TO.rows(O.ratio(self.sums[0]), n, apix)
        self.randomized_unmasked = TO.rows(O.ratio(self.sums[1]), n, apix)
        self.plain, self.spec = [self._stored(F) for F in bins], [self._stored(S) for S in subst]
        cw, sw = c2r_tables(n, fault)
        self.maps = []
        for S in self.spec:
            G = np.fft.ifft2(S.astype(np.complex128), axes=(0, 1))
            y = (G.real @ cw + G.imag @ sw).astype(np.float32)
            if fault == "map_last_rows":
                y.reshape(n * n, n)[-4:] = 0
            self.maps.append(y)

    def _stored(self, F):
        n = self.n
        S = F.copy()
        if self.fault == "spec_last_rows":
            S.reshape(n * n, n // 2 + 1)[-4:] = 0
        elif self.fault == "column_32":
            S[:, :, 32] = 0
        elif self.fault == "ky_rows_swapped":
            S[:, [1, 2]] = S[:, [2, 1]]
        return S

    def randomized_map(self, which, return_fft=False):
        return self.spec[which] if return_fft else self.maps[which]

    def _pair_sums(self, x, y, per_shell):
        if per_shell:
            return weighted_half_sums(x, y, self.n, 2.0 if self.fault == "full_sums_nyquist_weight_2" else 1.0)
        return O.sums_3d(x, y, False)

    def masked_sums(self, masks1, masks2=None, per_shell=False):
        m1 = np.asarray(masks1, dtype=np.float32)
        m2 = m1 if masks2 is None else np.asarray(masks2, dtype=np.float32)
        return np.stack([np.stack([self._pair_sums(self.a * p, self.b * q, per_shell),
                                   self._pair_sums(self.maps[0] * p, self.maps[1] * q, per_shell)]) for p, q in zip(m1, m2)])

    def masked(self, mask1, mask2=None, per_shell=False):
        s = self.masked_sums(np.asarray(mask1)[None], None if mask2 is None else np.asarray(mask2)[None], per_shell)[0]
        if per_shell:
            return O.ratio(s[0]), O.ratio(s[1])
        return TO.rows(O.ratio(s[0]), self.n, self.apix), TO.rows(O.ratio(s[1]), self.n, self.apix)

    def true_fsc(self, mask1, mask2=None):
        t, nz = self.masked(mask1, mask2)
        return np.column_stack((t[:, 0], TO.corrected(t[:, 1], nz[:, 1], self.cutoff_index)))

    def close(self):
        pass


__all__ = ["SIDES", "GENERATOR_SIDES", "GENERATOR_SEED", "FAULT_SIDES", "APIX", "TOL_FSC_3D", "TOL_ROUND_TRIP", "TOL_AMP", "TOL_ANGLE",
           "TRANSFORM_FACTOR", "FLOOR", "FAULTS", "q_of", "cutoff", "inputs", "masks", "oracle", "residues", "preconditions",
           "preconditions_hold", "compare", "exceeded", "figure_line", "philox4x32_10", "philox_angles", "generator_figures",
           "weighted_half_sums", "c2r_tables", "ModelTrueFSC", "sequential_dc"]
