"""The caps tests/test_gpu_launch_cuts.py crosses are the ones compiled into the library.

That file builds its lists from one table, CAPS.  This test reads the .inc files and asserts that every constant and every
`min` expression that decides a launch cut still has the table's value: a raised cap fails here instead of quietly turning a
three-launch list into one launch (and the GPU tests into tests of the first chunk alone)."""
import re
from pathlib import Path

from tests.test_gpu_launch_cuts import CAPS, chunks, spans_the_cap

CSRC = Path(__file__).resolve().parent.parent / "helicon_amd" / "csrc"


def source(name):
    """The file with comments dropped and white space collapsed."""
    text = re.sub(r"//[^\n]*", "", (CSRC / name).read_text())
    return re.sub(r"\s+", " ", text)


def constant(text, name):
    """The value of `constexpr int64_t NAME = <integer or (int64_t)a << b>;`, which must be defined exactly once."""
    found = re.findall(rf"constexpr int64_t {name} = ([^;]+);", text)
    assert len(found) == 1, (name, found)
    m = re.fullmatch(r"(?:\(int64_t\))?(\d+)(?: << (\d+))?", found[0].strip())
    assert m, (name, found[0])
    return int(m.group(1)) << int(m.group(2) or 0)


def test_zoom_and_phase_sweep_cap():
    zoom, phase = source("zoom_sweep.inc"), source("phase_sweep.inc")
    assert constant(zoom, "ZS_BATCH") == CAPS["ZS_BATCH"] == 8192
    cut = "const int64_t cap = std::min<int64_t>(n_cand, ZS_BATCH);"
    assert zoom.count(cut) == 1 and phase.count(cut) == 1
    for text in (zoom, phase):
        assert "for (int64_t b0 = 0; b0 < n_cand; b0 += cap) {" in text
        assert "ZS_BATCH =" not in text.replace("constexpr int64_t ZS_BATCH =", "")      # no second definition, no override


def test_filtered_sweep_caps():
    text = source("filtered_sweep.inc")
    assert constant(text, "FS_BATCH") == CAPS["FS_BATCH"] == 1024
    assert constant(text, "FS_BYTES") == CAPS["FS_BYTES"] == 128 * 1024 * 1024
    assert "const int64_t fit = std::max<int64_t>(1, FS_BYTES / (int64_t)((1 + J) * plane * sizeof(float)));" in text
    assert "const int64_t cap = std::min<int64_t>(n_cand, std::min<int64_t>(fit, FS_BATCH));" in text
    assert "for (int64_t b0 = 0; b0 < n_cand; b0 += cap) {" in text
    # the branch of the min each GPU case takes (J: 2 operator pairs on even sides, 4 on odd ones)
    assert CAPS["FS_BYTES"] // (3 * 16 * 16 * 4) > CAPS["FS_BATCH"]
    assert CAPS["FS_BYTES"] // (3 * 128 * 128 * 4) == 682 and CAPS["FS_BYTES"] // (5 * 127 * 127 * 4) == 416
    assert "if (ony % 2 == 1 && onx % 2 == 1) {" in text and text.count("++terms;") == 2


def test_fourier_correlation_caps():
    text = source("fourier_correlation.inc")
    assert CAPS["GRID_Z"] == 65535 and CAPS["FSC_MAPS_PER_PAIR"] == 2 and CAPS["FRC_PAIRS"] == 32767
    assert "chunk = std::min<int64_t>(chunk, p.cube ? 65535 / (2 * p.nz) : 32767);" in text
    assert "return std::min<int64_t>(chunk, batch);" in text
    assert "for (int64_t b0 = 0; b0 < batch; b0 += chunk) {" in text
    # the scratch cap is not what cuts the GPU tests' lists: 10 (cubes) or 6 (images) maps of float32 per pair
    scratch = constant(text, "FC_SCRATCH_BYTES")
    assert "const int64_t bytes_per_pair = (int64_t)(p.cube ? 10 : 6) * p.per_map * (int64_t)sizeof(float);" in text
    assert scratch // (10 * 8**3 * 4) > CAPS["GRID_Z"] // (2 * 8) == 4095
    assert scratch // (6 * 8 * 8 * 4) > CAPS["FRC_PAIRS"]


def test_true_fsc_cap():
    text = source("true_fsc.inc")
    assert CAPS["TFSC_MAPS_PER_MASK"] == 4
    assert "int64_t chunk = std::max<int64_t>(1, FC_SCRATCH_BYTES / (20 * per_map * (int64_t)sizeof(float)));" in text
    assert "chunk = std::min<int64_t>(chunk, 65535 / (4 * c->n));" in text
    assert "chunk = std::min<int64_t>(chunk, batch);" in text
    assert "for (int64_t b0 = 0; b0 < batch; b0 += chunk) {" in text
    scratch = constant(source("fourier_correlation.inc"), "FC_SCRATCH_BYTES")
    assert scratch // (20 * 8**3 * 4) > CAPS["GRID_Z"] // (4 * 8) == 2047


def test_symmetry_search_cap():
    text = source("symmetry_search.inc")
    assert CAPS["HS_CANDIDATES"] == CAPS["GRID_Z"] == 65535
    assert ("const size_t per_launch = (size_t)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(p->budget / (int64_t)per_cand), g, "
            "65535}));") in text
    assert "for (int64_t g0 = 0; g0 < g; g0 += (int64_t)per_launch) {" in text


def test_the_lists_of_the_gpu_tests_span_their_caps():
    assert chunks(17161, CAPS["ZS_BATCH"]) == [8192, 8192, 777] and spans_the_cap(17161, CAPS["ZS_BATCH"]) == [8192, 16384]
    assert chunks(2500, CAPS["FS_BATCH"]) == [1024, 1024, 452]
    assert chunks(1500, 682) == [682, 682, 136] and chunks(900, 416) == [416, 416, 68]
    assert chunks(8230, CAPS["GRID_Z"] // (CAPS["FSC_MAPS_PER_PAIR"] * 8)) == [4095, 4095, 40]
    assert chunks(32807, CAPS["FRC_PAIRS"]) == [32767, 40]
    assert chunks(4131, CAPS["GRID_Z"] // (CAPS["TFSC_MAPS_PER_MASK"] * 8)) == [2047, 2047, 37]
    assert chunks(65792, CAPS["HS_CANDIDATES"]) == [65535, 257]
