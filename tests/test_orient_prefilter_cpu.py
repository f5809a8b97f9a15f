"""CPU: the certain-drop test in front of the orientation launch (modsx_debug_reproject_certain_drop) against the oracle.

A region the test flags must be removed by the oracle's ReprojectRegions after EVERY rotation DetectOrientation could apply
to it: seeded regions around the four borders of the original image are rotated by 720 evenly spaced angles and by the f32
neighbours of 0, +-pi/2 and +-pi (f32 cos / sin, f64 products, as detect_orientation_batch forms them), reprojected by the
oracle under the identity and under the H of synthesised views of tilt 1, 2, 4 and 8, and no flagged region may be among the
survivors of any angle."""
import numpy as np
import pytest

W, H = 1024, 768
K_SIGMA = 2 * 3.0 * 3.0 ** 0.5      # synth-detection.cpp:28
N_PER_BORDER = 90
N_BAD = 12


def _angles():
    a = [np.arange(720, dtype=np.float64) * (2 * np.pi / 720) - np.pi]
    for v in (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi):
        f = np.float32(v)
        a.append(np.array([np.nextafter(f, np.float32(-4)), f, np.nextafter(f, np.float32(4))], np.float64))
    return np.concatenate(a).astype(np.float32)


def _half_box(s):
    return np.ceil(np.trunc(K_SIGMA * s) / 2.0)        # check_borders' hw of res_w = (int)(k_sigma * s)


def _regions(oracle, Hm, seed):
    """Regions of a view with homography Hm (view <- original): centres within +-3 hw of a border of the ORIGINAL image (a sixth
    of them further out, beyond the image), mapped into the view; s in 0.8 .. 40; A = R1 diag(q, 1 / q) R2 with q^2 <= 8.  The last
    N_BAD carry a NaN or an inf."""
    rs = np.random.RandomState(seed)
    n = 4 * N_PER_BORDER + N_BAD
    s = np.exp(rs.uniform(np.log(0.8), np.log(40.0), n))
    hw = _half_box(s)
    off = rs.uniform(-3, 3, n) * np.maximum(hw, 1.0)
    xo, yo = rs.uniform(0, W, n), rs.uniform(0, H, n)
    b = np.arange(n) % 4
    xo = np.where(b == 0, off, np.where(b == 1, W - 3 + off, xo))
    yo = np.where(b == 2, off, np.where(b == 3, H - 3 + off, yo))
    q = np.exp(rs.uniform(-0.5, 0.5, n) * np.log(8.0))
    t1, t2 = rs.uniform(0, 2 * np.pi, n), rs.uniform(0, 2 * np.pi, n)
    c1, s1, c2, s2 = np.cos(t1), np.sin(t1), np.cos(t2), np.sin(t2)
    # R1 diag(q, 1/q) R2
    a11 = c1 * q * c2 - s1 / q * s2
    a12 = -c1 * q * s2 - s1 / q * c2
    a21 = s1 * q * c2 + c1 / q * s2
    a22 = -s1 * q * s2 + c1 / q * c2
    assert np.allclose(a11 * a22 - a12 * a21, 1.0)
    regs = np.zeros(n, oracle.REGION)
    k = regs["det_kp"]
    k["x"] = Hm[0, 0] * xo + Hm[0, 1] * yo + Hm[0, 2]
    k["y"] = Hm[1, 0] * xo + Hm[1, 1] * yo + Hm[1, 2]
    k["a11"], k["a12"], k["a21"], k["a22"], k["s"] = a11, a12, a21, a22, s
    bad = np.arange(n - N_BAD, n)
    fields = ("x", "y", "a11", "a12", "a21", "a22", "s")
    for j, i in enumerate(bad):
        k[fields[j % len(fields)]][i] = (np.nan, np.inf, -np.inf)[j % 3]
    regs["id"] = np.arange(n)
    return regs, bad


def _rotated(regs, ang):
    """every region under every angle: cosf / sinf of the negated f32 angle, f64 products (engine.hip detect_orientation_batch)"""
    ci = np.cos(-ang).astype(np.float32).astype(np.float64)[None, :]
    si = np.sin(-ang).astype(np.float32).astype(np.float64)[None, :]
    out = np.repeat(regs, len(ang)).reshape(len(regs), len(ang))
    b = regs["det_kp"]
    b11, b12, b21, b22 = (b[f][:, None] for f in ("a11", "a12", "a21", "a22"))
    k = out["det_kp"]
    with np.errstate(invalid="ignore"):
        k["a11"] = b11 * ci - b12 * si
        k["a12"] = b11 * si + b12 * ci
        k["a21"] = b21 * ci - b22 * si
        k["a22"] = b21 * si + b22 * ci
    return out.reshape(-1)


@pytest.fixture(scope="module")
def homographies(oracle):
    views = oracle.set_vs_pars([1.0], [1, 2, 4, 8], 360.0, 0.5, 1, [])
    pick = {}
    for v in views:                                   # per tilt: the first and the last rotation of the ladder
        pick.setdefault(abs(v.tilt), []).append(v)
    assert sorted(pick) == [1.0, 2.0, 4.0, 8.0]
    gray = np.full((H, W), 128.0, np.float32)
    out = [("identity", np.eye(3))]
    for t in sorted(pick):
        for v in (pick[t][0], pick[t][-1]) if len(pick[t]) > 1 else (pick[t][0],):
            _, Hm, ident = oracle.synth_view(gray, v)
            out.append(("tilt %g phi %.3f" % (v.tilt, v.phi), Hm))
    return out


def test_no_flagged_region_survives_any_angle(modsx, oracle, homographies):
    ang = _angles()
    assert len(ang) == 720 + 15
    classes = dict(centre=0, left=0, right=0, top=0, bottom=0, sometimes=0, always=0)
    for vi, (name, Hm) in enumerate(homographies):
        regs, bad = _regions(oracle, Hm, 100 + vi)
        flag = modsx.reproject_certain_drop(regs.view(modsx.REGION), Hm, W, H)
        assert flag.dtype == bool and len(flag) == len(regs)
        assert not flag[bad].any(), name                  # NaN / inf anywhere: not certain
        kept = oracle.reproject_regions(_rotated(regs, ang), Hm, W, H)
        survived = np.bincount(kept["id"], minlength=len(regs))
        worst = np.flatnonzero(flag & (survived > 0))
        assert len(worst) == 0, (name, worst[:5], survived[worst[:5]], regs[worst[:5]])
        # what the flags were raised for, restated in f64 without a margin
        good = np.ones(len(regs), bool)
        good[bad] = False
        k = regs["det_kp"]
        eye = np.abs(Hm - np.eye(3)).sum() < 0.01
        Hi = np.eye(3) if eye else np.linalg.inv(Hm)
        hw = _half_box(np.where(good, k["s"], 1.0))
        with np.errstate(invalid="ignore"):
            x = Hi[0, 0] * k["x"] + Hi[0, 1] * k["y"] + Hi[0, 2]
            y = Hi[1, 0] * k["x"] + Hi[1, 1] * k["y"] + Hi[1, 2]
            dx = hw * np.hypot(Hi[0, 0] * k["a11"] + Hi[0, 1] * k["a21"], Hi[0, 0] * k["a12"] + Hi[0, 1] * k["a22"])
            dy = hw * np.hypot(Hi[1, 0] * k["a11"] + Hi[1, 1] * k["a21"], Hi[1, 0] * k["a12"] + Hi[1, 1] * k["a22"])
        with np.errstate(invalid="ignore"):
            inside = (x > 0) & (y > 0) & (x < W) & (y < H)
            classes["centre"] += int((flag & good & ~inside).sum())
            classes["left"] += int((flag & inside & (x - dx < 1)).sum())
            classes["right"] += int((flag & inside & (x + dx > W - 3)).sum())
            classes["top"] += int((flag & inside & (y - dy < 1)).sum())
            classes["bottom"] += int((flag & inside & (y + dy > H - 3)).sum())
        classes["sometimes"] += int((~flag & good & (survived > 0) & (survived < len(ang))).sum())
        classes["always"] += int((~flag & good & (survived == len(ang))).sum())
        # a region outside the image or over a border by more than a pixel in the restated bound is caught: the margin is a
        # fraction of a pixel
        with np.errstate(invalid="ignore"):
            clear = good & (~inside | (x - dx < 0) | (x + dx > W - 2) | (y - dy < 0) | (y + dy > H - 2))
        assert flag[clear].all(), name
    assert all(v > 0 for v in classes.values()), classes


def test_box_factor_and_bad_arguments(modsx, oracle):
    """the box factor is the caller's (ReprojectRegionsAndRemoveTouchBoundary uses mrSize): a smaller box flags fewer regions"""
    regs, bad = _regions(oracle, np.eye(3), 7)
    wide = modsx.reproject_certain_drop(regs.view(modsx.REGION), np.eye(3), W, H)
    narrow = modsx.reproject_certain_drop(regs.view(modsx.REGION), np.eye(3), W, H, boxk=3.0 * 3.0 ** 0.5)
    assert narrow.sum() < wide.sum() and not (narrow & ~wide).any()
    assert len(modsx.reproject_certain_drop(regs[:0].view(modsx.REGION), np.eye(3), W, H)) == 0
    none = modsx.reproject_certain_drop(regs.view(modsx.REGION), np.full((3, 3), np.nan), W, H)
    assert not none.any()
