"""Float64 NumPy oracle of the sweep's phase score across the meridian (hh_set_spectrum_phase).

Centre-origin DFT matrices at the scored plane's frequencies ``fftfreq(on) * 2 apix / cutoff``:
    F  = Ey @ img @ Ex.T            F~ = conj(Ey) @ img @ Ex.T        (the transform at (-f_y, f_x): across the meridian)
    c  = Re(F conj F~) / (|F| |F~|), 0 where the denominator is 0;    q = log1p|F| or |F|;    M = q c
    phase score = cosine_similarity(M_exp[mask], M_cand[mask])        (oracle.path_b, analysis.py:802-821)
all on the fftshifted plane.  The amplitude part is oracle.path_b's: compute_power_spectra + cross_correlation_coefficient."""
import numpy as np

from oracle import path_b as O


def transforms(img, apix=1.0, cutoff=None, size=None):
    """(F, F~) on the fftshifted ``size`` plane (default: the image's shape and Nyquist)."""
    img = np.asarray(img, dtype=np.float64)
    ny, nx = img.shape
    cy, cx = cutoff if cutoff is not None else (2 * apix, 2 * apix)
    ony, onx = size if size is not None else (ny, nx)
    fy = np.fft.fftfreq(ony) * 2 * apix / cy
    fx = np.fft.fftfreq(onx) * 2 * apix / cx
    ey = np.exp(-2j * np.pi * np.outer(fy, np.arange(ny) - ny // 2))   # [ony, ny]
    ex = np.exp(-2j * np.pi * np.outer(fx, np.arange(nx) - nx // 2))   # [onx, nx]
    f = ey @ img @ ex.T
    ft = np.conj(ey) @ img @ ex.T
    return np.fft.fftshift(f), np.fft.fftshift(ft)


def cos_across_meridian(f, ft):
    den = np.abs(f) * np.abs(ft)
    return np.divide((f * np.conj(ft)).real, den, out=np.zeros(f.shape), where=den > 0)


def phase_map(img, apix=1.0, cutoff=None, size=None, log=True):
    """(M, c, |F|) of one image."""
    f, ft = transforms(img, apix, cutoff, size)
    c = cos_across_meridian(f, ft)
    q = np.log1p(np.abs(f)) if log else np.abs(f)
    return q * c, c, np.abs(f)


def scores(img, params, mask, apix, d, br, cutoff=None, size=None, log=True, **geom):
    """(amplitude Pearson, phase score) of every candidate [twist, rise, csym, rot] against ``img``, float64."""
    ny, nx = np.shape(img)
    mask = np.asarray(mask, dtype=bool)
    img = np.asarray(img, dtype=np.float64)
    e = O.compute_power_spectra(img, apix, cutoff, size, log=log)[0]
    m_exp = phase_map(img, apix, cutoff, size, log)[0]
    amp, ph = [], []
    for tw, rs, cs, rot in params:
        sim = O.simulate_helical_projection(1, tw, rs, int(cs), d, br, 0, 0, ny, nx, apix, rot=rot, **geom)
        amp.append(O.cross_correlation_coefficient(e[mask], O.compute_power_spectra(sim, apix, cutoff, size, log=log)[0][mask]))
        ph.append(O.cosine_similarity(m_exp[mask], phase_map(sim, apix, cutoff, size, log)[0][mask]))
    return np.array(amp, dtype=np.float64), np.array(ph, dtype=np.float64)
