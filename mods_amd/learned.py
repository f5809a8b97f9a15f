"""Learned descriptors: the reference's "CAFFE" branch (imagerepresentation.cpp:1343-1534) with a torch module as the network.

Plain glue around three library entries: Context.caffe_patches writes the network's input blob into a torch tensor, the module
runs on the same device, Context.caffe_norm_rows_device normalises its output rows in place.  The rows never leave HBM; hand
the returned tensor's data_ptr() to Rep.append_f32_device.  The library entries return only after their own work has finished,
and torch's stream is synchronised before a pointer goes back to the library, so no stream is shared.
"""
import numpy as np

from . import CAFFE_NORM_L2, CAFFE_NORMS, REGION, caffe_params


def describe_learned(ctx, planes, regs, model, par=None, norm=CAFFE_NORM_L2, batch=256):
    """[n][dim] float32 rows on the context's device (a torch tensor) for the regions' reproj_kp on the original image.

    planes: one Image (gray) or three (B, G, R); regs: regions after reproject_regions; model: a callable that maps the
    [b][3][P][P] blob to [b][...] features, flattened here to [b][dim]; norm: CAFFE_NORM_* or the `Normalization=` name; batch:
    regions per forward pass (the reference's batchSize is 256; unlike the reference no batch sees the sums of earlier ones)."""
    import torch
    par = par or caffe_params()
    norm = CAFFE_NORMS[norm] if isinstance(norm, str) else int(norm)
    if batch < 1:
        raise ValueError("describe_learned: batch must be at least 1")
    regs = np.ascontiguousarray(regs, REGION)
    dev = torch.device("cuda", ctx.device)
    P = par.patchSize
    out = []
    with torch.no_grad():
        for b0 in range(0, len(regs), batch):
            part = regs[b0:b0 + batch]
            blob = torch.empty((len(part), 3, P, P), dtype=torch.float32, device=dev)
            ctx.caffe_patches(planes, part, par, out_ptr=blob.data_ptr())
            rows = model(blob).reshape(len(part), -1).to(torch.float32).contiguous()
            if rows.data_ptr() == blob.data_ptr():
                rows = rows.clone()
            torch.cuda.synchronize(dev)
            ctx.caffe_norm_rows_device(rows.data_ptr(), rows.shape[0], rows.shape[1], norm)
            out.append(rows)
    if not out:
        return torch.empty((0, 0), dtype=torch.float32, device=dev)
    return out[0] if len(out) == 1 else torch.cat(out)
