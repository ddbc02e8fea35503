"""-m gpu: every launch path of the predict / likelihood pipeline against the extended-precision reference.

Each case of tests/path_cases.py names the path it is there for; the host dispatch rules restated there, with the
device's CU count, say which paths gpemu_gp_predict and gpemu_logpost must take, and gpemu_path_counts deltas show that
they did.  On adversarial queries (training rows at the tile edges, 1e-7 length scales beside them, the general-nu
Bessel routine's t = 2 switch, far outside the design, walkers on the box edge) every element must lie within the
a-priori bound of tests/hp_ref.py: |dev - ref| <= bound, per element.  The reference runs on the subset of columns that
holds every special and edge column.
"""
import ctypes as C
import math

import numpy as np
import pytest

import golden_util as GU
import hp_ref as H
import path_cases as PC
from gpemu import _lib
from gpemu.sampler import DeviceSampler
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

LD = np.longdouble


def counts():
    out = np.zeros(len(PC.PATHS), dtype=np.int64)
    n = _lib.lib().gpemu_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    assert n == len(PC.PATHS), "enum gpemu_path and tests/path_cases.PATHS disagree"
    return out


def wide_counts():
    """gpemu_wide_path_counts beside the 8-wide KSTAR_KSTEPS2 / 3 counters: the keys of path_cases.wide_paths"""
    out = np.zeros(len(PC.WIDE_PATHS), dtype=np.int64)
    n = _lib.lib().gpemu_wide_path_counts(out.ctypes.data_as(C.POINTER(C.c_int64)), out.size)
    assert n == len(PC.WIDE_PATHS), "enum gpemu_wide_path and tests/path_cases.WIDE_PATHS disagree"
    c = counts()
    got = {"WIDE_" + p: int(v) for p, v in zip(PC.WIDE_PATHS, out)}
    got.update(KSTAR_KSTEPS2=int(c[PC.PATH["KSTAR_KSTEPS2"]]), KSTAR_KSTEPS3=int(c[PC.PATH["KSTAR_KSTEPS3"]]))
    return got


def assert_wide(w0, expected, what):
    got = {p: v - w0[p] for p, v in wide_counts().items()}
    assert got == expected, f"{what}: k-step / wide counts {got}, expected {expected}"


def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def within(what, dev, ref, bound):
    dev = np.asarray(dev, dtype=np.float64)
    err = np.abs(dev.astype(LD) - ref).astype(np.float64)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, (f"{what}: max err/bound {ratio.max():.3g} at {worst}: dev {dev[worst]!r} "
                                f"ref {float(ref[worst])!r} bound {bound[worst]:.3g}")
    return float(ratio.max())


def assert_paths(delta, expected, what):
    missing = [p for p in sorted(expected) if delta[PC.PATH[p]] == 0]
    assert not missing, f"{what}: paths not taken {missing}; deltas {dict(zip(PC.PATHS, delta.tolist()))}"


CASES = PC.cases(256)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_path_against_extended_reference(idx):
    ncu = num_cu()
    c = PC.cases(ncu)[idx]
    model, lo, hi, y_exp, y_err, bs, rng = PC.problem(c)
    Xq, rep, cols = PC.queries(c, model, lo, hi, rng)
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
    X = Xq[cols]
    mean, var, mb, vb, _ = pred = H.gp_predict(X, model, input_rounding=c.ls_bounds)
    lp, lb, _ = H.log_posterior(X, model, lo, hi, y_exp, y_err, bs, pred=pred)

    c0, w0 = counts(), wide_counts()
    m, v = dm.gp_predict(Xq)
    d_pred = counts() - c0
    assert_wide(w0, PC.wide_paths(c), c.name + " gp_predict")
    assert_paths(d_pred, PC.predict_paths(c, ncu), c.name + " gp_predict")
    assert d_pred[PC.PATH["PREDICT_PASS"]] == math.ceil(c.B / PC.MAX_CHUNK)
    ratios = {"mean": within("mean", m[cols], mean, mb), "var": within("var", v[cols], var, vb)}
    # the same query at the edge columns of every tile: the same arithmetic in every column of a pass, the same bits.
    # A column in a later pass of MAX_CHUNK rows (B = 2049: column 2048 alone) goes through the shape that pass has --
    # another cross-kernel row split, so another order of the mean's partial sums: it is held to the bound above only.
    same = rep[rep // PC.MAX_CHUNK == rep[0] // PC.MAX_CHUNK]
    for a in (m, v):
        assert np.array_equal(a[same], np.broadcast_to(a[same[0]], a[same].shape)), "repeated query differs across columns"

    c0, w0 = counts(), wide_counts()
    out0 = dm.logpost(Xq, mode=0)
    d_lp = counts() - c0
    if c.d > PC.DPAD:                      # (8-wide: the small half-step forms K_* without the cross-kernel launch)
        assert_wide(w0, PC.wide_paths(c), c.name + " logpost")
    assert_paths(d_lp, PC.logpost_paths(c, ncu), c.name + " logpost")
    out1 = dm.logpost(Xq, mode=1)
    lp64 = np.asarray(lp, dtype=np.float64)
    fin = np.isfinite(lp64)
    for out, mode in ((out0, 0), (out1, 1)):
        assert np.array_equal(np.isfinite(out[cols]), fin) and np.all(out[cols][~fin] == -np.inf), f"mode {mode}: -inf rows"
        if fin.any():
            ratios[f"lp{mode}"] = within(f"logpost mode {mode}", out[cols][fin], lp[fin], lb[fin])

    # predict_full on a few rows: central value and the diagonal of the covariance
    rows = cols[:3]
    cv, cov = dm.predict_full(Xq[rows], n_div=1.0)
    k = model.n_pc
    comp = model.components[:k].astype(LD)
    s = model.scaler_scale.astype(LD)
    cu = np.diag(O.cov_unexplained(model)).astype(LD)
    mr, vr, mbr, vbr = mean[:3], var[:3], mb[:3], vb[:3]
    cv_ref = (mr @ comp) * s + model.scaler_mean.astype(LD)
    ac = np.abs(model.components[:k]) * model.scaler_scale
    cv_b = mbr @ ac + 16 * H.U * (np.abs(np.asarray(mr, float)) @ ac + np.abs(model.scaler_mean))
    dg_ref = (vr @ (comp * comp)) * s * s + cu * s * s
    ac2 = ac * ac
    dg_b = vbr @ ac2 + 16 * H.U * (np.asarray(vr, float) @ ac2 + np.abs(np.asarray(cu, float)) * model.scaler_scale ** 2)
    ratios["cv"] = within("predict_full central value", cv, cv_ref, cv_b)
    ratios["cov"] = within("predict_full cov diagonal", np.diagonal(cov, axis1=1, axis2=2), dg_ref, dg_b)
    print(f"\nRATIOS {c.name} " + " ".join(f"{n}={r:.3g}" for n, r in ratios.items()))
    dm.close()


def _sampler_models(ng, seed, d=3):
    """ng single-block groups over the same d parameters (one kernel), set up for the sampler"""
    out = []
    for g in range(ng):
        c = PC.Case(f"g{g}", 40 + 7 * g, d, 3 + g % 3, 64, O.MATERN, 1.5, g % 2 == 1)
        model, lo, hi, y_exp, y_err, bs, _ = PC.problem(c, seed=seed)
        out.append((model, y_exp, y_err, bs))
    lo, hi = np.full(d, -2.0), np.full(d, 3.5)
    return out, lo, hi


def _groups_in_the_sampler(ng, d):
    """the state after 3 steps within the summed bounds; at d > 8 a quarter of the walkers start beside the upper box
    edge on the coordinates >= 8 only, so that stretch proposals leave the box there and nowhere else, and the whole
    chain must stay inside the box (with finite log-probabilities)"""
    groups, lo, hi = _sampler_models(ng, seed=ng, d=d)
    dms = []
    for model, y_exp, y_err, bs in groups:
        dm = GU.device_model(model)
        dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0)
        dms.append(dm)
    W = 64
    rng = np.random.default_rng(5)
    X0 = rng.uniform(-1.0, 1.0, (W, d))
    if d > PC.DPAD:
        X0[: W // 4, PC.DPAD:] = hi[PC.DPAD:] - rng.uniform(0.01, 0.1, (W // 4, d - PC.DPAD))
    ds = DeviceSampler(dms, W, seed=11)
    c0 = counts()
    ds.set_state(X0)
    ds.run(3)
    assert counts()[PC.PATH["LOGLIK_GROUPS"]] > c0[PC.PATH["LOGLIK_GROUPS"]]
    chain, lps = ds.get_chain()
    assert np.all((chain > lo) & (chain < hi)) and np.all(np.isfinite(lps)), "a walker left the box"
    X, lpd = ds.get_state()
    tot, bnd = np.zeros(W, dtype=LD), np.zeros(W)
    for model, y_exp, y_err, bs in groups:
        lp, lb, _ = H.log_posterior(X, model, lo, hi, y_exp, y_err, bs)
        tot += lp
        bnd += lb
    r = within(f"{ng}-group sampler state (d = {d})", lpd, tot, bnd)
    ds.close()
    for dm in dms:
        dm.close()
    return r


@pytest.mark.parametrize("ng", [3, 8])
def test_groups_kernel_in_the_sampler(ng):
    """several groups (up to LL_GROUPS_MAX = 8) in one likelihood launch: loglik_groups_kernel; the state's
    log-probabilities against the sum of the groups' references"""
    _groups_in_the_sampler(ng, 3)


def test_wide_groups_kernel_in_the_sampler():
    """three groups of 13 parameters (16-wide rows) in one loglik_groups_kernel launch, within the sum of the groups'
    bounds; walkers beside the box edge on lanes 8 .. 12 (_groups_in_the_sampler)"""
    r = _groups_in_the_sampler(3, 13)
    print(f"\nRATIOS wide_groups_d13 lp={r:.3g}")


def _blocks10(d=3):
    c = PC.Case("blocks10", 300, d, 5, 512, O.RBF, np.inf, False, nblk=10)
    return c, PC.problem(c)


def _fresh(model, y_exp, y_err, lo, hi, bs):
    dm = GU.device_model(model)
    dm.likelihood_setup(y_exp, y_err, lo, hi, 1.0, block_start=bs)
    return dm


def test_likelihood_state_across_calls():
    """logpost at B = 100, 600, 100, 2049 on one model (the tasks kernel's term buffer grows at 600 and 2049, the
    tickets are reset by the last workgroup of every row) equals, bit for bit, a freshly created model's"""
    c, (model, lo, hi, y_exp, y_err, bs, rng) = _blocks10()
    dm = _fresh(model, y_exp, y_err, lo, hi, bs)
    for B in (100, 600, 100, 2049):
        X = rng.uniform(lo, hi, (B, c.d))
        c0 = counts()
        got = dm.logpost(X)
        d = counts() - c0
        assert d[PC.PATH["LOGLIK_TASKS_MULTI"] if B <= 256 else PC.PATH["LOGLIK_TASKS_MULTI_BIG"]] > 0, B
        ref = _fresh(model, y_exp, y_err, lo, hi, bs)
        want = ref.logpost(X)
        ref.close()
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), f"B = {B}: differs from a fresh model"
    dm.close()


def test_sampler_10_blocks_with_and_without_tasks_kernel(monkeypatch):
    """a 10-block sampler with 1024 walkers (512 proposals per half-step: the tasks kernel above 256 rows) gives the
    chain of the serial likelihood kernel bit for bit, and a second run on the same model equals a fresh one"""
    _ten_blocks_with_and_without_tasks(monkeypatch, 3)


def test_wide_sampler_10_blocks_with_and_without_tasks_kernel(monkeypatch):
    """the same at 16 parameters: 16-wide proposals through the tasks kernel and through the serial one"""
    _ten_blocks_with_and_without_tasks(monkeypatch, 16)


def _ten_blocks_with_and_without_tasks(monkeypatch, d):
    c, (model, lo, hi, y_exp, y_err, bs, rng) = _blocks10(d)
    W = 1024
    X0 = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (W, c.d))
    chains = []
    for env in (None, "1"):
        if env is None:
            monkeypatch.delenv("GPEMU_NO_LOGLIK_TASKS", raising=False)
        else:
            monkeypatch.setenv("GPEMU_NO_LOGLIK_TASKS", env)
        dm = _fresh(model, y_exp, y_err, lo, hi, bs)
        ds = DeviceSampler([dm], W, seed=2024)
        c0 = counts()
        ds.set_state(X0)
        ds.run(5)
        delta = counts() - c0
        chain, lps = ds.get_chain()
        chains.append((chain, lps))
        if env is None:
            assert delta[PC.PATH["LOGLIK_TASKS_MULTI_BIG"]] > 0
            ds.run(5)                      # the same model and sampler again: tickets and terms as left behind
            ds.close()
            ds = DeviceSampler([dm], W, seed=2024)
            ds.set_state(X0)
            ds.run(5)
            again, lps2 = ds.get_chain()
            assert np.array_equal(again.view(np.int64), chain.view(np.int64))
            assert np.array_equal(lps2.view(np.int64), lps.view(np.int64))
        ds.close()
        dm.close()
    monkeypatch.delenv("GPEMU_NO_LOGLIK_TASKS", raising=False)
    assert np.array_equal(chains[0][0].view(np.int64), chains[1][0].view(np.int64))
    assert np.array_equal(chains[0][1].view(np.int64), chains[1][1].view(np.int64))
