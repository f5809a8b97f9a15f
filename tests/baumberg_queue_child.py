"""Child process of tests/test_gpu_baumberg_queue.py: detect_affine_keypoints on the small pair under whatever MODSX_BAUMBERG_QUEUE the
parent put into the environment (the switch is read once per process).  argv: output .npz.  Writes the production variant the
process reports and the keypoint records of both images as bytes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SMALL_PAIR = dict(rows=240, cols=320, nblobs=420, seed=777)        # tests/conftest.py small_pair


def detect(modsx, ctx, images):
    """-> list of KEYPOINT arrays: mode 0 (no export cut: every converged keypoint), and the default export of the pair path"""
    out = []
    for img in images:
        im = ctx.upload(img)
        out.append(ctx.detect_affine_keypoints(im, modsx.default_hessaff_params(mode=0, reg_number=1 << 20)))
        out.append(ctx.detect_affine_keypoints(im, modsx.default_hessaff_params()))
        im.free()
    return out


def main(outp):
    import mods_amd
    from mods_amd import synthetic
    a, b, _ = synthetic.make_pair(**SMALL_PAIR)
    ctx = mods_amd.Context(0)
    recs = detect(mods_amd, ctx, (a, b))
    ctx.close()
    np.savez(outp, variant=np.int32(mods_amd.baumberg_production_variant(19)),
             **{"k%d" % i: np.frombuffer(r.tobytes(), np.uint8) for i, r in enumerate(recs)})


if __name__ == "__main__":
    main(sys.argv[1])
