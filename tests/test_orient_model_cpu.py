"""CPU: tests/orient_model.py restates the oracle's dominant_angles bit for bit on every planted patch of tests/orient_cases.py, and
its pieces (mask, atan2LUT case / angle, the library's host tables) agree with the oracle and with mods_amd.orientation_tables()."""
import numpy as np
import pytest

import orient_cases as cases
import orient_model as M


def _same_angles(a, b):
    return len(a) == len(b) and np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("th", [0.8, 1.0, 0.5])
def test_model_equals_oracle_on_every_planted_patch(oracle, half, th):
    P = cases.planted()
    A = cases.analysis(oracle)
    for max_angles in (-1, 1, 2, 18):
        got, _ = M.dominant_angles_batch(oracle, None, half, th, max_angles, analysis=A)
        bad = [c["name"] for c, g in zip(P, got) if not _same_angles(g, oracle.dominant_angles(c["patch"], half, th, max_angles))]
        assert not bad, (half, th, max_angles, len(bad), bad[:5])


def test_max_angles_zero_gives_nothing(oracle):
    P = cases.planted()
    got, _ = M.dominant_angles_batch(oracle, None, 0, 0.8, 0, analysis=cases.analysis(oracle))
    assert all(len(g) == 0 for g in got)
    assert all(len(oracle.dominant_angles(c["patch"], 0, 0.8, 0)) == 0 for c in P[::97])


def test_single_patch_entry_and_report_shapes(oracle):
    c = cases.planted()[-1]
    ang, rep = M.dominant_angles(oracle, c["patch"], half=1, th=0.5, max_angles=2)
    assert _same_angles(ang, oracle.dominant_angles(c["patch"], 1, 0.5, 2))
    assert rep["bin"].shape == (41, 41) and rep["votes"].shape == (37,) and rep["raw"].shape == (37,)
    assert rep["smoothed"].shape == rep["folded"].shape == rep["peak"].shape == (36,) and rep["thresh"].shape == ()
    assert rep["votes"].sum() == (rep["bin"] >= 0).sum()


def test_atan_case_and_angle_equal_the_oracles_atan2lut(oracle):
    rs = np.random.RandomState(5)
    y = np.concatenate([rs.standard_normal(4000) * 30, [0, 0, 0, 3, -3, 1, 1, -1, -1, 2.5, -2.5, 0.0]]).astype(np.float32)
    x = np.concatenate([rs.standard_normal(4000) * 30, [0, 3, -3, 0, 0, 1, -1, 1, -1, 2.5, 2.5, -0.0]]).astype(np.float32)
    bx, by = cases.BIG_IDX255
    y, x = np.concatenate([y, [by, -by]]).astype(np.float32), np.concatenate([x, [bx, -bx]]).astype(np.float32)
    code, idx, special = M.atan_case(y, x)
    got = M.angle_of_case(oracle.atan_lut(), code, idx, special)
    want = np.array([oracle.atan2lut(float(a), float(b)) for a, b in zip(y, x)], np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert special[4000] and special[4004] and not special[4003] and idx[-1] == 255 and code[-2] == 7 and code[-1] == 1


def test_mask_and_voting_list(oracle, modsx):
    m = M.circular_gauss_mask()
    r, c = M.voting_list()
    assert len(r) == M.NVOTERS == 1245
    assert not m[0].any() and not m[-1].any() and not m[:, 0].any() and not m[:, -1].any()          # none on the frame
    assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1])
    t = modsx.orientation_tables()
    assert t["n_real"] == 1245 and t["length"] == 1344 == 64 * 21 and t["stride"] == 44 and t["global_table_from"] == 8192
    # the list is the model's mask in raster order, padded with weight 0 at pixel (1, 1)
    assert np.array_equal(t["index_raster"][:1245], (r * 44 + c).astype(np.uint16))
    assert np.array_equal(t["weight_raster"][:1245].view(np.int32), m[r, c].view(np.int32))
    assert (t["index_raster"][1245:] == 45).all() and not t["weight_raster"][1245:].any()
    rr, cc = t["index_raster"][:1245] // 44, t["index_raster"][:1245] % 44
    assert rr.min() >= 1 and rr.max() <= 39 and cc.min() >= 1 and cc.max() <= 39
    # the uploaded order: entry l + 64 q = list element 21 l + q
    lane, q = np.meshgrid(np.arange(64), np.arange(21), indexing="ij")
    assert np.array_equal(t["index_lanes"][lane + 64 * q], t["index_raster"][21 * lane + q])
    assert np.array_equal(t["weight_lanes"][lane + 64 * q], t["weight_raster"][21 * lane + q])


def test_bin_table_is_the_oracles_expression_for_every_entry(oracle, modsx):
    tab = modsx.orientation_tables()["bin_table"]
    assert tab.shape == (2049,)
    L = oracle.atan_lut()
    code, idx = np.divmod(np.arange(2048), 256)
    ang = M.angle_of_case(L, code, idx)
    assert np.array_equal(tab[:2048], M.bin_of_angle(ang).astype(np.uint8))
    assert tab[2048] == 18 == M.bin_of_angle(np.float32(0.0))
    assert tab.max() == 36 and tab.min() == 0 and (tab == 36).sum() == 1 and tab[3 * 256 + 0] == 36
    # each entry against the oracle's own atan2lut on a gradient that reaches it: (big, small) = (255, idx + 0.5), or (255, 255)
    PIf = np.float32(np.pi)
    for e in range(2048):
        c, i = divmod(e, 256)
        if i == 255 and c & 1:
            big, small = (float(v) for v in cases.BIG_IDX255)
        else:
            big, small = 255.0, (255.0 if i == 255 else i + 0.5)
        ax, ay = (big, small) if c & 1 else (small, big)
        x, y = (ax if c & 4 else -ax), (ay if c & 2 else -ay)
        ori = np.float32(oracle.atan2lut(y, x))
        assert tab[e] == int(np.float32(36) * (ori / PIf + np.float32(1.0)) / np.float32(2.0)), (c, i)
    assert tab[2048] == int(np.float32(36) * (np.float32(oracle.atan2lut(-3.0, 0.0)) / PIf + np.float32(1.0)) / np.float32(2.0))
