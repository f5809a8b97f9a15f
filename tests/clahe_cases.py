"""The inputs of the CLAHE tests: images (shape x content) and parameters (clip, grid, variant).  tests/test_clahe_cases_cpu.py
proves on the CPU, with tests/clahe_model.py, that the list reaches what it claims; tests/test_gpu_clahe.py runs the device on it.

Shapes are rows x cols; grids are (tiles_x, tiles_y).  ONE_STRIP / TWO_STRIPS lie on both sides of the two work-split rules of the
library at a 1 x 1 grid: 64 x 64 is one histogram strip per tile (64 rows of 64 = 4096 px) and one workgroup of the pixel pass
(4096 px), 65 x 64 is two of each."""
import functools

import numpy as np

from tests import clahe_model as M

SHAPES = [(2, 2), (8, 8), (9, 17), (64, 64), (100, 75), (135, 239), (131, 257)]
BIG = (768, 1024)
ONE_STRIP, TWO_STRIPS = (64, 64), (65, 64)
GRIDS = [(8, 8), (1, 1), (3, 5), (16, 16)]
CLIPS = [4.0, 40.0, 0.0, 0.01, 2.5]
TIE_SEED = 5           # the noise image of 64 x 64 whose interpolation at 8 x 8 lands on x.5 (tile 8 x 8: dyadic weights)


def content(kind, shape, seed=0):
    """the gray f32 image of one content kind"""
    rows, cols = shape
    y, x = np.mgrid[0:rows, 0:cols]
    if kind == "constant":
        return np.full(shape, 97.0, np.float32)
    if kind == "two_valued":
        return np.where(((y // 3) + (x // 5)) % 2 == 0, 40.0, 200.0).astype(np.float32)
    if kind == "hramp":
        return np.floor(x * 255.0 / max(cols - 1, 1)).astype(np.float32)
    if kind == "vramp":
        return np.floor(y * 255.0 / max(rows - 1, 1)).astype(np.float32)
    if kind == "noise":
        return np.random.RandomState(1000 + seed).randint(0, 256, shape).astype(np.float32)
    if kind == "smooth_noise":       # a narrow band of levels: most bins empty, the used ones far above the clip limit
        return (100 + np.random.RandomState(2000 + seed).randint(0, 12, shape)).astype(np.float32)
    if kind == "saturated_tile":     # the first tile of an 8 x 8 grid all 255 beside a flat 100
        img = np.full(shape, 100.0, np.float32)
        img[:max(rows // 8, 1), :max(cols // 8, 1)] = 255.0
        return img
    if kind == "f32_edges":          # k + 0.5 for even and odd k (ties of the u8 conversion), below 0, above 255, NaN, infinities
        vals = np.array([0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 253.5, 254.5, 255.5, -0.5, -0.49, -3.0, -1e30, 255.49, 256.0, 300.0, 1e30,
                         np.nan, np.inf, -np.inf, 10.25, 10.75, 77.0, 200.5000153], np.float32)
        idx = np.random.RandomState(3000 + seed).randint(0, len(vals), shape)
        return vals[idx]
    raise KeyError(kind)


CONTENTS = ["constant", "two_valued", "hramp", "vramp", "noise", "smooth_noise", "saturated_tile", "f32_edges"]


def _build():
    cases = []

    def add(shape, kind, clip, grid, variant, seed=0):
        cases.append(dict(shape=shape, kind=kind, clip=clip, grid=grid, variant=variant, seed=seed))

    # every small shape on every grid, both variants, the drivers' clip
    for shape in SHAPES + [TWO_STRIPS]:
        for grid in GRIDS:
            seed = len(cases)        # the two variants see the same image
            for variant in (0, 1):
                add(shape, "noise", 4.0, grid, variant, seed=seed)
    # every content, both variants, on a divisible, a padded and a tiny shape
    for shape in [(64, 64), (100, 75), (9, 17)]:
        for kind in CONTENTS:
            for variant in (0, 1):
                add(shape, kind, 4.0, (8, 8), variant)
    # every clip on three shapes, with content that the limit bites
    for shape in [(64, 64), (135, 239), (100, 75)]:
        for clip in CLIPS[1:]:
            for kind in ("smooth_noise", "noise"):
                for variant in (0, 1):
                    add(shape, kind, clip, (8, 8), variant)
    # one tile over the whole image: residual 0 (clipLimit 256 of 4096 px), 1 (255), 255 (1), and clipped < 256 (64 px)
    for variant in (0, 1):
        add((64, 64), "constant", 16.0, (1, 1), variant)
        add((64, 64), "constant", 15.99, (1, 1), variant)
        add((64, 64), "constant", 0.01, (1, 1), variant)
        add((8, 8), "constant", 4.0, (1, 1), variant)
        add((8, 8), "two_valued", 4.0, (3, 5), variant)       # 8 % 3 != 0: the columns are padded too
        add((8, 8), "noise", 4.0, (8, 3), variant)            # cols divisible, rows not: the columns get a whole grid
        add((64, 64), "noise", 4.0, (8, 8), variant, seed=TIE_SEED)
        add(ONE_STRIP, "noise", 4.0, (1, 1), variant, seed=7)
        add(TWO_STRIPS, "hramp", 40.0, (1, 1), variant)
        add((131, 257), "f32_edges", 2.5, (3, 5), variant)
    # the benchmark's size: three strips per tile at 8 x 8, 192 strips of one tile
    add(BIG, "noise", 4.0, (8, 8), 0, seed=11)
    add(BIG, "smooth_noise", 4.0, (8, 8), 1, seed=12)
    add(BIG, "vramp", 40.0, (1, 1), 0)
    return cases


CASES = _build()


def name(k):
    c = CASES[k]
    return "%d-%dx%d-%s-clip%g-grid%dx%d-v%d" % (k, c["shape"][0], c["shape"][1], c["kind"], c["clip"], c["grid"][0], c["grid"][1], c["variant"])


@functools.lru_cache(maxsize=None)
def image(k):
    c = CASES[k]
    img = content(c["kind"], c["shape"], c["seed"])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(k):
    """the model's stages for case k (computed once per process)"""
    c = CASES[k]
    return M.run(image(k), c["clip"], c["grid"], c["variant"])


SMALL = [k for k, c in enumerate(CASES) if c["shape"] != BIG]
# the mixed-size batch at the drivers' parameters: one image per small shape and the big one
BATCH = [k for k, c in enumerate(CASES) if c["kind"] == "noise" and c["clip"] == 4.0 and c["grid"] == (8, 8) and c["variant"] == 0
         and (c["seed"] == k or c["shape"] == BIG)]
