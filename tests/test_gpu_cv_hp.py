"""-m gpu sweep of cross-validation on the device (csrc/k_cv.hip, DeviceModel.cross_validate) against the
extended-precision reference of tests/cv_hp_ref.py: for every admitted case of tests/cv_cases.py the four outputs
(mean_pc, var_pc, central_value, variance), element by element, within the a-priori bound; none NaN, no variance negative.

Measured on one MI355X: per conditioning class the largest, over its cases, of max |device - reference| / bound (the
lines this module prints with -s):

    class (cases)      mean_pc   var_pc   central_value   variance
    noise 5e-2 (20)    0.29      0.024    0.27            0.51
    noise 1e-4 (7)     0.041     0.016    0.22            0.45
    noise-free (13)    0.48      0.037    0.22            0.45

The largest mean_pc figures are leave-one-out calls (loo_n63 0.29, loo_n129_m05_free 0.48), whose bound is a few ulp;
the factored path stays below 0.04 in PC space (the float64 host run of the same algorithm: the same), and the
back-projection, whose bound counts its k + 2 and 2 k + 3 roundings one by one, reaches 0.51.  The bounds themselves:
at noise 5e-2 at most 3.4e-12 max|y| (mean) and 7.3e-12 var (m = 129, RBF), at the noise-free RBF sweep case
(cond(L) = 6.6e4) 1.3e-10 max|y| and 1.0e-9 var.  A library with u scaled by 1 + 1e-11 in cv_u_kernel fails 34 of the
40 sweep cases here (the 6 leave-one-out calls form no u) and passes test_gpu_cross_validation.py.
"""
import numpy as np
import pytest

import cv_cases as CC
import cv_hp_ref as H
import golden_util as GU

pytestmark = pytest.mark.gpu

ADMITTED = [c.name for c in CC.cases()]
DUPS = [c.name for c in CC.cases() if c.data.startswith("dup")]
MANY_PCS = next(c.name for c in CC.cases() if c.k >= 11)


def _run(name):
    model, y, fold, _ = CC.build(name)
    dm = GU.device_model(model)
    try:
        return dm.cross_validate(y, fold)
    finally:
        dm.close()


def _check(name, out, what=""):
    ref = CC.reference(name)
    r = H.ratios(out, ref)
    print(f"{name}{what} [{CC.case(name).conditioning}] max err / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    bad = H.violations(out, ref)
    assert not bad, f"{name}{what}: " + "; ".join(bad)
    return ref


@pytest.mark.parametrize("name", ADMITTED)
def test_device_inside_the_bound(name):
    _check(name, _run(name))


def test_chunks_straddling_folds_give_the_same_bits(monkeypatch):
    """k >= 11 PCs, three folds: chunks of 3 problems hold problems of two folds, at the reference-checked level"""
    one = _run(MANY_PCS)
    monkeypatch.setenv("GPEMU_CV_CHUNK", "3")
    many = _run(MANY_PCS)
    for a, b in zip(one, many):
        assert a.tobytes() == b.tobytes()
    _check(MANY_PCS, many, " (chunks of 3)")


@pytest.mark.parametrize("name", DUPS)
def test_clipped_points_are_the_reference_s(name):
    """var == 0 exactly where the reference clips; a point whose unclipped reference value lies within its bound of 0
    may fall on either side"""
    out = _run(name)
    ref = _check(name, out)
    raw = ref.var_raw.astype(np.float64)
    decided = np.abs(raw) > ref.var_bound
    dev, want = out[1] == 0.0, raw < 0
    print(f"{name}: device clips {int(dev.sum())}, reference {int(want.sum())}, undecided {int((~decided).sum())}")
    assert np.array_equal(dev[decided], want[decided])
    if CC.case(name).data == "dup_split_pivot":
        assert want.any()
