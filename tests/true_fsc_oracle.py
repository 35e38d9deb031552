"""NumPy / SciPy restatement of the reference's phase-randomised true FSC (lib/filters.py:469-520 randomize_phases_lowpass,
commands/trueFSC.py:102-366), the yardstick of tests/test_gpu_true_fsc.py, itself pinned to the reference's recorded output
by tests/golden/g20_true_fsc.npz (tests/test_true_fsc_host.py).  Built on tests/fsc_oracle.py; the package under test is not
imported."""
import numpy as np

import fsc_oracle as O


def reference_cutoff_mask(n, apix, cutoff_res):
    """filters.py:505-510: the reference's float64 expression of the randomised set on the half spectrum."""
    cutoff_freq2 = (apix / cutoff_res) ** 2
    k, kr = np.fft.fftfreq(n), np.fft.rfftfreq(n)
    k2, kr2 = k * k, kr * kr
    return (k2[:, None, None] + k2[None, :, None] + kr2[None, None, :]) >= cutoff_freq2


def m_half(n):
    """kz^2 + ky^2 + kx^2 of the half spectrum's bins, folded integer frequencies."""
    f = np.rint(np.fft.fftfreq(n) * n).astype(np.int64)
    return f[:, None, None] ** 2 + f[None, :, None] ** 2 + f[None, None, : n // 2 + 1] ** 2


def randomize_phases_lowpass(data, apix, cutoff_res, return_fft, draws):
    """filters.py:469-520 with the uniform draws given (the reference takes them from np.random), in the input's own precision:
    on a float32 map this is the reference's complex64 output bit for bit."""
    from scipy.fft import irfftn, rfftn

    F = rfftn(data)
    amp, phase = np.abs(F), np.angle(F)
    mask = reference_cutoff_mask(data.shape[-1], apix, cutoff_res)
    random_phases = np.exp(1j * draws)
    phase[mask] = np.angle(random_phases[mask])
    out = amp * np.exp(1j * phase)
    return out if return_fft else irfftn(out)


def randomized_spectrum(data, m_cut, angles):
    """float64: the rfftn half spectrum with every bin of m >= m_cut replaced by |F| e^{i angle}; the other bins untouched."""
    F = np.fft.rfftn(np.asarray(data, dtype=np.float64))
    sel = m_half(F.shape[0]) >= m_cut
    F[sel] = np.abs(F[sel]) * np.exp(1j * np.asarray(angles, dtype=np.float64)[sel])
    return F


def irfftn(F):
    """scipy.fft.irfftn's semantics on a half spectrum that is not Hermitian-consistent, in float64."""
    from scipy.fft import irfftn as _irfftn

    return _irfftn(np.asarray(F, dtype=np.complex128))


def sums_of_spectra(F1, F2):
    n = F1.shape[0]
    return O.shell_sums(F1, F2, O.shell_3d_half(n), n // 2 + 1)


def rows(fsc, n, apix):
    saxis = np.arange(n // 2 + 1) * (1.0 / (apix * n))
    keep = np.where(saxis <= np.fft.rfftfreq(n).max())
    return np.vstack((saxis[keep], fsc[keep])).T


def find_resolution(saxis, fsc, threshold):
    """trueFSC.py:427-462."""
    idx = np.where(np.asarray(fsc) < threshold)[0]
    if len(idx) == 0:
        return 999.0
    i = idx[0]
    if i == 0:
        return 1.0 / saxis[0] if saxis[0] > 0 else 999.0
    x0, x1, y0, y1 = saxis[i - 1], saxis[i], fsc[i - 1], fsc[i]
    cross = x1 if y0 == y1 else x0 + (threshold - y0) * (x1 - x0) / (y1 - y0)
    return 999.0 if cross <= 0 else 1.0 / cross


def corrected(fsc_t, fsc_n, cutoff_index):
    """trueFSC.py:342-348."""
    out = np.copy(fsc_t)
    i = cutoff_index + 1
    with np.errstate(divide="ignore", invalid="ignore"):
        out[i:] = (fsc_t[i:] - fsc_n[i:]) / (1 - fsc_n[i:])
    out[np.isnan(out)] = 1.0
    return out


def sphere_mask(n, radius, edge):
    """A soft spherical mask: 1 inside `radius`, a raised cosine over `edge` voxels, 0 outside."""
    g = np.arange(n) - n // 2
    r = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    return np.clip(0.5 * (1 + np.cos(np.pi * np.clip((r - radius) / edge, 0, 1))), 0, 1)


class OracleTrueFSC:
    """helicon_amd.true_fsc.TrueFSC's interface in float64 on the host (`cutoff_res` must be given: > 2).  `m_cut` follows the
    integer rule; the tests assert that it selects the reference expression's bins for their cutoffs."""

    def __init__(self, map1, map2, apix, cutoff_res, *, phases=None, seed=None, device=0, m_cut=None):
        assert cutoff_res > 2 and phases is not None and seed is None
        self.a, self.b = np.asarray(map1, dtype=np.float64), np.asarray(map2, dtype=np.float64)
        self.n, self.apix, self.cutoff_res = self.a.shape[0], float(apix), float(cutoff_res)
        n = self.n
        self.cutoff_index = int(n * apix / cutoff_res)
        if m_cut is None:
            m_cut = int(np.ceil((apix / cutoff_res) ** 2 * n * n - 1e-9))
        self.m_cut = m_cut
        self.F1r, self.F2r = randomized_spectrum(self.a, m_cut, phases[0]), randomized_spectrum(self.b, m_cut, phases[1])
        self.ar, self.br = irfftn(self.F1r), irfftn(self.F2r)
        self.sums = np.stack([O.sums_3d(self.a, self.b), sums_of_spectra(self.F1r, self.F2r)])
        self.unmasked = rows(O.ratio(self.sums[0]), n, apix)
        self.randomized_unmasked = rows(O.ratio(self.sums[1]), n, apix)

    def masked_sums(self, masks1, masks2=None, per_shell=False):
        m1 = np.asarray(masks1, dtype=np.float64)
        m2 = m1 if masks2 is None else np.asarray(masks2, dtype=np.float64)
        return np.stack([np.stack([O.sums_3d(self.a * p, self.b * q, per_shell), O.sums_3d(self.ar * p, self.br * q, per_shell)])
                         for p, q in zip(m1, m2)])

    def masked(self, mask1, mask2=None, per_shell=False):
        s = self.masked_sums(np.asarray(mask1)[None], None if mask2 is None else np.asarray(mask2)[None], per_shell)[0]
        if per_shell:
            return O.ratio(s[0]), O.ratio(s[1])
        return rows(O.ratio(s[0]), self.n, self.apix), rows(O.ratio(s[1]), self.n, self.apix)

    def true_fsc(self, mask1, mask2=None):
        t, nz = self.masked(mask1, mask2)
        return np.column_stack((t[:, 0], corrected(t[:, 1], nz[:, 1], self.cutoff_index)))

    def close(self):
        pass
