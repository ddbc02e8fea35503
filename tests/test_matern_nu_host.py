"""CPU tests of the Matern kernel of general smoothness nu: the restatement (tests/matern_nu_ref.py) against the goldens
the reference made (tests/golden/make_goldens_matern_nu.py), the device's Bessel routine (csrc/matern_dev.h) built for
the host against scipy.special.kv, and the Python stand-ins' handling of nu (nu = inf -> the RBF kind; nu <= 0 / NaN
refused before any library call)."""
import math
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import golden_util as GU
import matern_nu_ref as R
from oracle import gp_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SINGLE = ["g8_matern_nu_0p75", "g8_matern_nu_2p0", "g8_matern_nu_3p5", "g8_matern_nu_inf"]


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("name", SINGLE)
def test_restatement_reproduces_the_reference(name):
    g = GU.load(name)
    spec = GU.spec_of(g)
    X = g["design"]
    assert relerr(R.kernel_matrix(X, g["theta"][0], spec), g["kernel_matrix_pc0"]) < 1e-12
    ytr = g["Y_pca_truncated"]
    for i in range(int(g["n_pc"])):
        assert abs(R.lml(X, ytr[:, i], g["theta"][i], spec) - g["lml_at_theta"][i]) < 1e-10 * abs(g["lml_at_theta"][i])
    with R.general_nu():
        model = GU.group_model(g)
        m, v = O.gp_predict_all(g["Xq"], model)
        pg = O.predict_group(g["Xq"], model)
        lp = O.log_posterior(g["Xw"], {"g": model}, g["lo"], g["hi"], g["y_exp"], g["y_err"])
        lp1 = np.array([O.log_posterior(x, {"g": model}, g["lo"], g["hi"], g["y_exp"], g["y_err"])[0] for x in g["Xw"]])
    assert relerr(m, g["gp_mean"]) < 1e-10
    assert np.max(np.abs(v - g["gp_var"])) < 1e-10 * max(1.0, np.max(g["gp_var"]))
    assert relerr(pg["central_value"], g["batch_central_value"]) < 1e-10
    assert relerr(pg["cov"][:g["batch_cov_head"].shape[0]], g["batch_cov_head"]) < 1e-10
    assert relerr(lp, g["logpost_batched"]) < 1e-10
    assert relerr(lp1, g["logpost_per_walker"]) < 1e-10
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))          # (the last two queries lie far outside)


# observables of the three-group golden (make_goldens_matern_nu.py): {observable: (group, output slice, group slice)}
MAPPING3 = {"A": ("g1", slice(0, 10), slice(0, 10)), "B": ("g2", slice(10, 18), slice(0, 8)),
            "C": ("g3", slice(18, 30), slice(0, 12))}


def test_restatement_reproduces_the_reference_three_groups():
    g = GU.load("g8_matern_nu_3groups")
    groups = ("g1", "g2", "g3")
    with R.general_nu():
        models = {n: GU.group_model(g, prefix=n + "_") for n in groups}
        mapping = MAPPING3
        go = {n: O.predict_group(g["Xq"], models[n]) for n in groups}
        merged = O.merge_groups(go, mapping, g["Y"].shape[1])
        lp = O.log_posterior(g["Xw"], models, g["lo"], g["hi"], g["y_exp"], g["y_err"], mapping=mapping)
    assert relerr(merged["central_value"], g["merged_central_value"]) < 1e-10
    assert relerr(merged["cov"][:2], g["merged_cov_head"]) < 1e-10
    assert relerr(lp, g["logpost_batched"]) < 1e-10


def test_device_bessel_routine_on_the_host_matches_scipy(tmp_path):
    """csrc/matern_dev.h compiled for the CPU: t^nu K_nu(t), t^nu K_(nu-1)(t) and the kernel value against scipy over
    t in [1e-8, 700] (scipy's own error reaches ~5e-14 next to t = 2)"""
    from scipy.special import gamma, kve
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "matern_nu_check"
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "native", "matern_nu_check.cpp"),
                    "-o", str(exe)], check=True)
    nus = [0.05, 0.3, 0.49, 0.5, 0.51, 0.75, 1.0, 1.0005, 1.3, 2.0, 2.5, 3.5, 4.2, 7.0]
    ts = np.concatenate([np.geomspace(1e-8, 700, 120), [1.999999, 2.0, 2.0000001]])
    inp = "\n".join(f"{nu!r} {float(t)!r}" for nu in nus for t in ts)
    out = np.array([[float(v) for v in line.split()]
                    for line in subprocess.run([str(exe)], input=inp, capture_output=True, text=True,
                                               check=True).stdout.split("\n") if line])
    i = 0
    for nu in nus:
        for t in ts:
            kn, km, val = out[i]
            i += 1
            # (compared times e^t: scipy's unscaled kv underflows to 0 near t = 700)
            et = np.exp(t)
            rn, rm = t ** nu * kve(nu, t), t ** nu * kve(nu - 1, t)
            assert abs(kn * et - rn) <= 2e-13 * rn, (nu, t, kn, rn)
            assert abs(km * et - rm) <= 2e-13 * rm, (nu, t, km, rm)
            rv = 2 ** (1 - nu) / gamma(nu) * rn
            assert abs(val * et - rv) <= 2e-13 * rv, (nu, t, val, rv)
    # the edges: r = 0 gives 1, a large distance gives 0 (not NaN)
    res = subprocess.run([str(exe)], input="0.75 0\n2.0 0\n0.75 1e5\n3.5 1e4\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert float(res[0].split()[2]) == 1.0 and float(res[1].split()[2]) == 1.0
    assert float(res[2].split()[2]) == 0.0 and float(res[3].split()[2]) == 0.0


class _FakeLib:
    """records the arguments of the create calls; every call succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def fake_lib(monkeypatch):
    from gpemu import _lib
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    monkeypatch.setattr(_lib, "resolve_device", lambda d=None: 0)
    return fake


def test_nu_inf_goes_to_the_device_as_the_rbf_kind(fake_lib):
    from gpemu import fit as _fit
    from gpemu.model import DeviceModel
    X = np.random.default_rng(0).uniform(size=(20, 3))
    _fit.DeviceFit(X, 1, np.inf, True, True)
    _fit.DeviceFit(X, 1, 2.0, True, True)
    _fit.kernel_matrix(X, np.zeros(3), 1, np.inf)
    k, N = 2, 20
    DeviceModel(X, np.ones((k, 3)), np.zeros((k, N)), np.tile(np.eye(N), (k, 1, 1)), np.ones((k, 5)), np.zeros(5),
                np.ones(5), kernel_kind=1, nu=math.inf)
    DeviceModel(X, np.ones((k, 3)), np.zeros((k, N)), np.tile(np.eye(N), (k, 1, 1)), np.ones((k, 5)), np.zeros(5),
                np.ones(5), kernel_kind=1, nu=0.75)
    got = [(n, a) for n, a in fake_lib.calls if n in ("gpemu_fit_create", "gpemu_kernel_matrix", "gpemu_model_create")]
    fit_inf, fit_2, km_inf, mod_inf, mod_075 = [a for _, a in got]
    assert (fit_inf[5], fit_inf[6]) == (0, 0.0)          # kernel_kind, nu
    assert (fit_2[5], fit_2[6]) == (1, 2.0)
    assert (km_inf[6], km_inf[7]) == (0, 0.0)
    assert (mod_inf[6], mod_inf[7]) == (0, 0.0)
    assert (mod_075[6], mod_075[7]) == (1, 0.75)


def test_nu_inf_stays_in_kernel_():
    from gpemu import estimators as E
    k = E.ARDKernel(E.MATERN_KIND, [1.0, 2.0], [[0.01, 100]] * 2, nu=math.inf, noise_level=0.1,
                    noise_level_bounds=(1e-3, 10))
    assert k.nu == math.inf and "nu=inf" in repr(k) and k.kind == E.MATERN_KIND
    k2 = pickle.loads(pickle.dumps(k))
    assert k2.nu == math.inf and repr(k2) == repr(k)
    assert k.clone().nu == math.inf
    k3 = E.ARDKernel(E.MATERN_KIND, [1.0], [[0.01, 100]], nu=2.0)
    assert "nu=2" in repr(k3)


@pytest.mark.parametrize("nu", [0.0, -1.5, float("nan"), -math.inf])
def test_bad_nu_is_refused_before_any_library_call(nu, fake_lib):
    from gpemu import _lib
    from gpemu import estimators as E
    from gpemu import fit as _fit
    with pytest.raises(ValueError):
        E.ARDKernel(E.MATERN_KIND, [1.0], [[0.01, 100]], nu=nu)
    with pytest.raises(ValueError):
        _lib.kernel_args(1, nu)
    with pytest.raises(ValueError):
        _fit.DeviceFit(np.zeros((4, 2)), 1, nu)
    assert fake_lib.calls == []


def test_bad_nu_in_the_config_is_refused():
    import types

    from bayesian_inference import emulation
    cfg = types.SimpleNamespace(
        analysis_config={"parameterization": {"p": {"min": [0.0, 0.0], "max": [1.0, 1.0]}}}, parameterization="p",
        active_kernels={"matern": {"length_scale_bounds_factor": [0.01, 100], "nu": -0.5}})
    with pytest.raises(ValueError):
        emulation.build_kernel(cfg)
    cfg.active_kernels["matern"]["nu"] = float("inf")
    k = emulation.build_kernel(cfg)
    assert k.nu == math.inf
