"""CPU-side checks of the ImageNet-C style corruption family's interface: the three new symbols and the fav_corruption_desc
layout (C vs ctypes), the severity table, the taps of the two blur kinds against their float64 definition, the pixelate
cell map, and robustness.summarize on hand-made arrays."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import corrupt_c_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from failure_aware_vision_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "fav.h"
int main(void) {
    printf("size %zu\n", sizeof(fav_corruption_desc));
#define F(x) printf("d.%s %zu\n", #x, offsetof(fav_corruption_desc, x));
    F(struct_size) F(kind) F(a) F(b) F(seed) F(first_frame_index)
    printf("kinds %d %d %d %d %d %d %d %d %d\n", (int)FAV_C_IMPULSE_NOISE, (int)FAV_C_SPECKLE_NOISE, (int)FAV_C_GAUSSIAN_BLUR,
           (int)FAV_C_DEFOCUS_BLUR, (int)FAV_C_CONTRAST, (int)FAV_C_PIXELATE, (int)FAV_C_BRIGHTNESS, (int)FAV_C_SATURATE,
           (int)FAV_C_COUNT);
    printf("abi %d\n", (int)FAV_ABI_VERSION);
    return 0;
}
"""


def test_layout_symbols_and_abi(lib, tmp_path):
    from failure_aware_vision_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).splitlines()
    out = {ln.split()[0]: ln.split()[1:] for ln in lines}
    assert int(out["size"][0]) == 32 == C.sizeof(_lib.FavCorruptionDesc)
    for name in ("struct_size", "kind", "a", "b", "seed", "first_frame_index"):
        assert int(out["d." + name][0]) == getattr(_lib.FavCorruptionDesc, name).offset, name
    assert [int(v) for v in out["kinds"]] == list(range(9))
    assert _lib.CORRUPTION_KINDS == R.KINDS
    for sym in ("fav_corruption_params", "fav_corruption_taps", "fav_op_corrupt_c"):
        assert hasattr(lib, sym), sym
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for sym in ("fav_corruption_params(", "fav_corruption_taps(", "fav_op_corrupt_c("):
        assert sym in header, sym
    assert int(out["abi"][0]) == 2 == lib.fav_abi_version()


def test_severity_table(lib):
    from failure_aware_vision_amd import CORRUPTIONS, SEVERITY
    from failure_aware_vision_amd.synth import GAUSSIAN_NOISE_SIGMA
    for k, kind in enumerate(R.KINDS):
        for sev in range(1, 6):
            a, b = C.c_float(-1), C.c_float(-1)
            assert lib.fav_corruption_params(k, sev, C.byref(a), C.byref(b)) == 0
            want = R.TABLE[kind][sev - 1]
            assert (a.value, b.value) == (float(f32(want[0])), float(f32(want[1]))), (kind, sev)
            assert SEVERITY[kind][sev - 1] == (a.value, b.value)
    a, b = C.c_float(-1), C.c_float(-1)
    for kind, sev in ((0, 0), (0, 6), (-1, 3), (8, 3)):
        assert lib.fav_corruption_params(kind, sev, C.byref(a), C.byref(b)) == 1, (kind, sev)
        assert b"fav_corruption_params" in lib.fav_last_error(None)
        assert (a.value, b.value) == (-1.0, -1.0)
    assert lib.fav_corruption_params(0, 1, None, C.byref(b)) == 1
    assert CORRUPTIONS == R.KINDS + ("gaussian_noise",) and set(SEVERITY) == set(CORRUPTIONS)
    assert SEVERITY["gaussian_noise"] == tuple((float(s), 0.0) for s in GAUSSIAN_NOISE_SIGMA)


def ulp(x):
    return np.spacing(np.abs(x).astype(f32)).astype(np.float64)


@pytest.mark.parametrize("severity", (1, 2, 3, 4, 5))
def test_gaussian_taps(lib, severity):
    a, b = R.params("gaussian_blur", severity)
    st, taps, rad = R.lib_taps(lib, "gaussian_blur", a, b)
    want, Rw = R.gauss_taps_f64(a)
    assert st == 0 and rad == Rw == R.GAUSS_RADII[severity - 1] and taps.shape == (2 * rad + 1,)
    assert (np.abs(taps.astype(np.float64) - want) <= ulp(want)).all()
    assert abs(taps.astype(np.float64).sum() - 1.0) <= taps.size * 2.0 ** -24
    assert np.array_equal(taps, taps[::-1])
    st, none, _ = R.lib_taps(lib, "gaussian_blur", a, b, cap=2 * rad)
    assert st == 1 and none is None and b"fav_corruption_taps" in lib.fav_last_error(None)


@pytest.mark.parametrize("severity", (1, 2, 3, 4, 5))
def test_defocus_taps(lib, severity):
    a, b = R.params("defocus_blur", severity)
    st, taps, rad = R.lib_taps(lib, "defocus_blur", a, b)
    want, Rw = R.disk_taps_f64(a, b)
    S = 2 * rad + 1
    assert st == 0 and rad == Rw == R.DEFOCUS_RADII[severity - 1] and taps.shape == (S, S)
    assert (np.abs(taps.astype(np.float64) - want) <= ulp(want)).all()
    assert abs(taps.astype(np.float64).sum() - 1.0) <= taps.size * 2.0 ** -24
    assert np.array_equal(taps, taps.T) and np.array_equal(taps, taps[::-1]) and np.array_equal(taps, taps[:, ::-1])
    assert taps[0, 0] == 0.0 and taps[rad, rad] > 0.0
    st, none, _ = R.lib_taps(lib, "defocus_blur", a, b, cap=S * S - 1)
    assert st == 1 and none is None and b"fav_corruption_taps" in lib.fav_last_error(None)


def test_taps_rejections(lib):
    buf, rad = (C.c_float * 4096)(), C.c_int32()
    for kind in ("impulse_noise", "speckle_noise", "contrast", "pixelate", "brightness", "saturate"):
        assert R.lib_taps(lib, kind, 0.5, 0.0)[0] == 1, kind                   # no taps
    for kind, a, b in (("gaussian_blur", 0.0, 0.0), ("gaussian_blur", -1.0, 0.0), ("gaussian_blur", 8.2, 0.0),
                       ("gaussian_blur", math.nan, 0.0), ("gaussian_blur", math.inf, 0.0), ("defocus_blur", 0.5, 0.5),
                       ("defocus_blur", 13.0, 0.5), ("defocus_blur", 3.0, 0.0), ("defocus_blur", 3.0, math.nan)):
        assert R.lib_taps(lib, kind, a, b)[0] == 1, (kind, a, b)
    assert R.lib_taps(lib, "gaussian_blur", 8.1, 0.0)[2] == 32                  # the largest radius
    assert R.lib_taps(lib, "defocus_blur", 12.9, 0.5)[2] == 14
    assert lib.fav_corruption_taps(2, 1.0, 0.0, None, 4096, C.byref(rad)) == 1
    assert lib.fav_corruption_taps(2, 1.0, 0.0, buf, 4096, None) == 1
    assert lib.fav_corruption_taps(8, 1.0, 0.0, buf, 4096, C.byref(rad)) == 1


def test_pixelate_cell_map():
    """The properties of the map itself, on the reference's restatement (corrupt_c_ref.cell_map): this does not run the
    library's cell_start / cellof, which the GPU file's bit-exact pixelate test compares with this map."""
    for H in range(1, 41):
        for c, _ in R.TABLE["pixelate"]:
            hd, cell = R.cell_map(H, c)
            assert 1 <= hd <= H and hd == max(1, int(float(H) * float(f32(c))))
            assert np.array_equal(np.unique(cell), np.arange(hd)), (H, c)        # every cell occurs
            assert (np.diff(cell) >= 0).all()


def test_summarize():
    from failure_aware_vision_amd import risk_coverage, summarize
    from failure_aware_vision_amd.robustness import COLUMNS, table
    labels = np.array([0, 1, 2, 3, 4, 5])
    conf = np.array([0.9, 0.8, 0.3, 0.6, 0.2, 0.95], f32)
    nll = np.array([0.1, 0.2, 1.5, 0.5, 2.0, 0.05], f32)
    mixed = np.array([0, 1, 9, 3, 9, 9])                                       # frames 2, 4 and 5 wrong
    s = summarize(mixed, conf, nll, labels, 0.5)                                # flagged: frames 2 and 4
    assert s["accuracy"] == 0.5 and s["fail_rate"] == 2 / 6
    assert s["error_recall"] == 2 / 3 and s["flag_precision"] == 1.0
    assert s["mean_confidence"] == pytest.approx(float(conf.astype(np.float64).mean()), abs=1e-15)
    assert s["nll"] == pytest.approx(float(nll.astype(np.float64).mean()), abs=1e-15)
    assert s["aurc"] == risk_coverage(conf, mixed == labels)["aurc"]
    assert set(s) == set(COLUMNS)
    s = summarize(labels, conf, nll, labels, 0.5)                               # all correct
    assert s["accuracy"] == 1.0 and math.isnan(s["error_recall"]) and s["flag_precision"] == 0.0 and s["aurc"] == 0.0
    s = summarize(labels + 1, conf, nll, labels, 0.5)                           # all wrong
    assert s["accuracy"] == 0.0 and s["error_recall"] == 2 / 6 and s["flag_precision"] == 1.0 and s["aurc"] == 1.0
    s = summarize(mixed, conf, nll, labels, 0.0)                                # nothing flagged
    assert s["fail_rate"] == 0.0 and s["error_recall"] == 0.0 and math.isnan(s["flag_precision"])
    s = summarize(mixed, conf, nll, labels, 2.0)                                # everything flagged
    assert s["fail_rate"] == 1.0 and s["error_recall"] == 1.0 and s["flag_precision"] == 0.5
    s = summarize(labels, conf, nll, labels, 0.0)                               # nothing wrong, nothing flagged
    assert math.isnan(s["error_recall"]) and math.isnan(s["flag_precision"])
    assert summarize(mixed, conf, nll, labels, conf[3])["fail_rate"] == 2 / 6   # conf == tau is not flagged
    with pytest.raises(ValueError):
        summarize(mixed[:3], conf, nll, labels, 0.5)
    text = table({("clean", 0): summarize(labels, conf, nll, labels, 0.5), ("contrast", 3): summarize(mixed, conf, nll, labels, 0.5)})
    assert len(text.splitlines()) == 4 and "contrast" in text and "nan" in text
