"""CPU: the case list of the external affine adaptation tests (tests/affshape_cases.py) is fit for its purpose, and the host's
share of DetectAffineShape (mods_amd.affshape_jobs: ratio, truncated window argument, up-front border test) is right.
tests/test_gpu_affshape.py compares the device path with tests/affshape_model.py region by region on these cases; this module
proves without a device, from the oracle's reports, that the cases reach what such a comparison has to reach.
"""
import numpy as np
import pytest

from tests import affshape_cases as AC
from tests import affshape_model as AM


@pytest.fixture(scope="module")
def exp(oracle):
    return AC.expected(oracle)


def _all(exp, f):
    return np.concatenate([rep[f] for _, rep in exp])


def test_shapes_and_sizes(oracle):
    ims, regs = AC.images(oracle), AC.regions()
    assert [im.shape for im in ims] == [(48, 64), (61, 97), (19, 23)] and all(im.dtype == np.float32 for im in ims)
    assert 300 <= sum(len(r) for r in regs) <= 700
    for r in regs:
        AM.assert_f32_scales(r)
        assert r.dtype.itemsize == 200
    assert (ims[1][:, :AC.FLAT_COLS] == 90.0).all()


def test_fitness_shares(exp):
    """a test on these cases cannot pass on an empty result: >= 30 % pass the border test, >= 20 % converge"""
    border, reason = _all(exp, "border"), _all(exp, "reason")
    n = len(border)
    print(n, (~border).mean(), (reason == 0).mean())
    assert (~border).sum() >= 0.3 * n and (reason == 0).sum() >= 0.2 * n
    assert sum(len(out) for out, _ in exp) == (reason == 0).sum()
    for (out, rep), regs in zip(exp, AC.regions()):
        assert np.array_equal(out["id"], regs["id"][rep["reason"] == 0])          # order is kept


def test_every_exit_and_touch_class_is_reached(exp):
    border, reason, touch = _all(exp, "border"), _all(exp, "reason"), _all(exp, "touch")
    count = np.bincount(reason[~border], minlength=5)
    print(count, np.bincount(touch[~border], minlength=4))
    assert count[0] >= 100 and count[1] >= 20 and count[2] >= 3 and count[3] >= 100 and count[4] >= 30
    assert (reason[border] == -1).all()
    # regions that pass the up-front test and still take interpolate()'s border branch inside the loop: always, never, sometimes
    t = np.bincount(touch[~border], minlength=4)
    assert t[0] == 0 and t[1] >= 30 and t[2] >= 100 and t[3] >= 30
    it = _all(exp, "iters")[reason == 0]
    assert len(set(it.tolist())) >= 8


def _corner_conditions(reg, rows, cols, res):
    """which of interpolateCheckBorders' four conditions fire on any corner, restated in numpy f32 (helpers.cpp:524-549)"""
    f = np.float32
    k = reg["det_kp"]
    half = f(np.ceil(f(res) / 2.0))
    fired = set()
    for sx, sy in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
        imx = f(f(f(k["x"]) + f(f(sx) * half) * f(k["a11"])) + f(f(sy) * half) * f(k["a12"]))
        imy = f(f(f(k["y"]) + f(f(sx) * half) * f(k["a21"])) + f(f(sy) * half) * f(k["a22"]))
        if np.floor(imx) <= 0:
            fired.add("left")
        if np.floor(imy) <= 0:
            fired.add("top")
        if np.ceil(imx) >= cols - 2:
            fired.add("right")
        if np.ceil(imy) >= rows - 2:
            fired.add("bottom")
    return fired


def test_each_corner_condition_refuses_alone(exp):
    for i, ((_, rep), regs) in enumerate(zip(exp, AC.regions())):
        rows, cols = AC.SHAPES[i]
        for side in ("left", "top", "right", "bottom"):
            k = AC.planted(i, side)
            assert rep["border"][k], (i, side)
            assert _corner_conditions(regs[k], rows, cols, rep["res"][k]) == {side}, (i, side)
        # and the restatement agrees with the oracle on every region of the list
        mine = np.array([bool(_corner_conditions(regs[k], rows, cols, rep["res"][k])) for k in range(len(regs))])
        assert np.array_equal(mine, rep["border"])


def test_identity_and_own_matrix_judge_differently(oracle, exp):
    for i, ((_, rep), regs) in enumerate(zip(exp, AC.regions())):
        rows, cols = AC.SHAPES[i]
        ident = regs.copy()
        ident["det_kp"]["a11"], ident["det_kp"]["a12"], ident["det_kp"]["a21"], ident["det_kp"]["a22"] = 1.0, 0.0, 0.0, 1.0
        bi, _, _ = AM.border_test(oracle, ident, rows, cols)
        a, b = AC.planted(i, "identity passes, own matrix refused"), AC.planted(i, "identity refused, own matrix passes")
        assert not bi[a] and rep["border"][a]
        assert bi[b] and not rep["border"][b]
        assert (bi != rep["border"]).sum() >= 5


def test_window_argument_steps(exp):
    for i, ((_, rep), regs) in enumerate(zip(exp, AC.regions())):
        for m in (1, 2, 7, 8):
            a, b = AC.planted(i, "step %d below" % m), AC.planted(i, "step %d on" % m)
            wa, wb = 10.0 * np.float64(rep["ratio"][a]), 10.0 * np.float64(rep["ratio"][b])
            assert m - 1e-5 < wa < m <= wb < m + 1e-5
            assert (rep["res"][a], rep["res"][b]) == (m - 1, m)
            # the two scales are neighbouring f32 numbers
            sa, sb = np.float32(regs["det_kp"]["s"][a]), np.float32(regs["det_kp"]["s"][b])
            assert np.nextafter(sa, np.float32(1e9)) == sb
            if m in (1, 7):      # ceil(res / 2) grows with this step, and the border test follows it
                assert not rep["border"][a] and rep["border"][b]
            else:
                assert not rep["border"][a] and not rep["border"][b]
        assert rep["res"][AC.planted(i, "step 1 below")] == 0
    res = _all(exp, "res")
    assert (res % 2 == 1).any() and (res % 2 == 0).any() and (res < 0).any()


def test_negative_scales_run(exp):
    s = np.concatenate([r["det_kp"]["s"] for r in AC.regions()])
    border, reason = _all(exp, "border"), _all(exp, "reason")
    neg = s < 0
    assert neg.sum() >= 10 and (neg & ~border).sum() >= 5 and (neg & (reason == 0)).sum() >= 1
    assert (_all(exp, "ratio")[neg] < 0).all()


def test_output_matrix_is_u_not_u_times_a(oracle, exp):
    """regions with a non-identity input matrix converge, and what they get is the U of the same region with the identity: the
    input orientation takes part in the border test only"""
    total = 0
    for i, ((out, rep), regs) in enumerate(zip(exp, AC.regions())):
        k = regs["det_kp"]
        nonid = (k["a11"] != 1.0) | (k["a12"] != 0.0) | (k["a21"] != 0.0) | (k["a22"] != 1.0)
        sel = np.nonzero(nonid & (rep["reason"] == 0))[0]
        total += len(sel)
        ident = regs[sel].copy()
        ident["det_kp"]["a11"], ident["det_kp"]["a12"], ident["det_kp"]["a21"], ident["det_kp"]["a22"] = 1.0, 0.0, 0.0, 1.0
        _, rep_i = AM.run(oracle, AC.images(oracle)[i], ident)
        ran = ~rep_i["border"]
        assert ran.sum() >= 0.5 * len(sel)
        assert np.array_equal(rep_i["u"][ran].view(np.uint32), rep["u"][sel][ran].view(np.uint32))
        got = out[np.isin(out["id"], regs["id"][sel])]
        U = rep["u"][sel].astype(np.float64)
        for j, f in enumerate(("a11", "a12", "a21", "a22")):
            assert np.array_equal(got["det_kp"][f], U[:, j])
        for f in ("x", "y", "s", "response"):
            assert np.array_equal(got["det_kp"][f], regs["det_kp"][f][sel])
        assert np.array_equal(got["reproj_kp"], regs["reproj_kp"][sel])
    assert total >= 50


def test_converged_and_dropped_regions_are_interleaved(exp):
    for i, (_, rep) in enumerate(exp):
        keep = rep["reason"] == 0
        changes = (keep[1:] != keep[:-1]).sum()
        assert changes >= (40 if i < 2 else 4), (i, changes)
    # and so are refused and launched ones: compaction of the job list is visible
    for _, rep in exp:
        assert (rep["border"][1:] != rep["border"][:-1]).sum() >= 10


def test_affshape_jobs_against_the_formulas(modsx, oracle):
    """mods_amd.affshape_jobs on 10^4 random regions whose scales are arbitrary doubles: ratio and res against the numpy formulas,
    the border test against the oracle's interpolateCheckBorders.  The f32 division the kernels use for scale-space keypoints
    gives another ratio for some of them: the count is asserted, this is the one place where such scales are checked."""
    rs = np.random.RandomState(424242)
    n = 10000
    rows, cols = 61, 97
    regs = np.zeros(n, modsx.REGION)
    k = regs["det_kp"]
    k["x"], k["y"] = rs.uniform(-3.0, cols + 3.0, n), rs.uniform(-3.0, rows + 3.0, n)
    k["s"] = np.where(rs.uniform(size=n) < 0.5, rs.uniform(0.05, 5.0, n), np.sqrt(rs.uniform(1.0, 700.0, n)))   # sqrt(size): the Saddle branch
    k["s"][::17] *= -1.0
    phi, k1, k2 = rs.uniform(0, np.pi, n), rs.uniform(0.05, 2.5, n), rs.uniform(0.05, 2.5, n)
    k["a11"], k["a12"], k["a21"], k["a22"] = np.cos(phi) * k1, -np.sin(phi) * k2, np.sin(phi) * k1, np.cos(phi) * k2
    k["a11"][::5], k["a12"][::5], k["a21"][::5], k["a22"][::5] = 1.0, 0.0, 0.0, 1.0
    got = modsx.affshape_jobs(regs, cols, rows)
    ratio, res = AM.ratio_res(k["s"])
    assert np.array_equal(got["ratio"].view(np.uint32), ratio.view(np.uint32))
    assert np.array_equal(got["res"], res)
    border, _, _ = AM.border_test(oracle, regs, rows, cols)
    assert np.array_equal(got["border"], border)
    assert min(border.sum(), n - border.sum()) >= 1000          # both answers of the border test are well represented
    not_f32 = k["s"].astype(np.float32).astype(np.float64) != k["s"]
    f32_division = k["s"].astype(np.float32) / (np.float32(1.6) * np.float32(1.0))
    differ = (f32_division.view(np.uint32) != ratio.view(np.uint32)).sum()
    print("scales that are no f32 numbers:", not_f32.sum(), "ratios the f32 division would change:", differ)
    assert not_f32.sum() > 0.9 * n and differ > 0
    # for f32 scales the two agree (what lets tests/affshape_model.py use the oracle's findAffineShape)
    s32 = k["s"].astype(np.float32)
    r32, _ = AM.ratio_res(s32.astype(np.float64))
    assert np.array_equal((s32 / np.float32(1.6)).view(np.uint32), r32.view(np.uint32))
