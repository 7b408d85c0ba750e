"""Chunked CPU reference of the convolution stack (conv_encoder / conv_decoder of dreamer_oracle.py) and the elementwise
error metric the GPU tests judge it by.

The encoder and the decoder are run a chunk of frames at a time (forward and backward), outputs are concatenated and
parameter gradients summed over the chunks, so memory stays bounded at production frame counts (2 500 frames).  The same
functions run in fp64 (the reference proper; chunk gradients are summed in fp64) and in fp32 (the "what does plain fp32
arithmetic give" run that sets each tensor's bar at run time; chunk gradients are summed in fp32, like everything else
in that run).

Metric per tensor:  err = max_i |got_i - ref64_i| / rms(ref64).  One wrong element of ordinary size gives err ~ 1, however
large the tensor is.  Bar per tensor:  max(10 * err_ref32, 64 * eps_fp32), err_ref32 being the same metric of the fp32 CPU
run (tests/test_gpu_conv_stack.py states where the factor and the floor come from).
"""
import numpy as np
import torch

from oracle import dreamer_oracle as O

ENC = 'wm.encoder.encoder_image.model'
DEC = 'wm.decoder.image.model'
BAR_FACTOR = 10.0
BAR_FLOOR = 64.0 * float(np.finfo(np.float32).eps)      # 7.6e-6


def to_frames(image, dtype):
    """Frames as the oracle wants them: float (N, C, H, W) in [-0.5, 0.5].  uint8 (N, H, W, C) frames are converted by the
    reference's x / 255 - 0.5 in `dtype`; float (N, C, H, W) frames are only cast."""
    if image.dtype == torch.uint8:
        return (image.to(dtype) / 255.0 - 0.5).permute(0, 3, 1, 2).contiguous()
    return image.to(dtype)


def _leaves(params, prefix, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items() if k.startswith(prefix + '.')}


def encoder_reference(params, image, dembed, dtype=torch.float64, chunk=128):
    """params: state-dict entries of the encoder; image: (N, C, 64, 64) float or (N, 64, 64, C) uint8; dembed: (N, E).
    Returns {'embed': (N, E), 'dW0'..'dW3', 'db0'..'db3'} in `dtype` (embed = conv_encoder(image), gradients of
    sum(embed * dembed))."""
    N = image.shape[0]
    p = _leaves(params, ENC, dtype)
    acc = {k: torch.zeros_like(v) for k, v in p.items()}
    embed = []
    for s in range(0, N, chunk):
        x = to_frames(image[s:s + chunk], dtype)
        out = O.conv_encoder(p, x[None])[0]
        grads = torch.autograd.grad(out, list(p.values()), dembed[s:s + chunk].to(dtype))
        for k, g in zip(p, grads):
            acc[k] += g
        embed.append(out.detach())
    res = {'embed': torch.cat(embed)}
    for i in range(4):
        res[f'dW{i}'] = acc[f'{ENC}.{2 * i}.weight'].detach()
        res[f'db{i}'] = acc[f'{ENC}.{2 * i}.bias'].detach()
    return res


def decoder_reference(params, feat, target, scale, row_scale=None, tdiv=1, dtype=torch.float64, chunk=128):
    """params: state-dict entries of the image decoder; feat: (N, F); target: (N / tdiv, C, 64, 64) float or
    (N / tdiv, 64, 64, C) uint8 - prediction frame n is compared with target frame n // tdiv (iwae_samples).
    loss_image[n] = 0.5 * sum (pred[n] - target[n // tdiv])^2; the gradients are those of
    sum_n scale * row_scale[n] * loss_image[n]  (row_scale = 1 when None).
    Returns {'image_rec': (N, C, 64, 64), 'loss_image': (N,), 'dfeat': (N, F), 'dW0'..'dW4', 'db0'..'db4'} in `dtype`."""
    N = feat.shape[0]
    p = _leaves(params, DEC, dtype)
    acc = {k: torch.zeros_like(v) for k, v in p.items()}
    rec, loss, dfeat = [], [], []
    idx = torch.arange(N) // tdiv
    for s in range(0, N, chunk):
        f = feat[s:s + chunk].detach().to(dtype).clone().requires_grad_(True)
        tg = to_frames(target[idx[s:s + chunk]], dtype)
        pred = O.conv_decoder(p, f)
        li = 0.5 * torch.square(pred - tg).sum(dim=[-1, -2, -3])
        w = torch.full((f.shape[0],), float(scale), dtype=dtype)
        if row_scale is not None:
            w = w * row_scale[s:s + chunk].to(dtype)
        grads = torch.autograd.grad((li * w).sum(), [f] + list(p.values()))
        dfeat.append(grads[0])
        for k, g in zip(p, grads[1:]):
            acc[k] += g
        rec.append(pred.detach())
        loss.append(li.detach())
    res = {'image_rec': torch.cat(rec), 'loss_image': torch.cat(loss), 'dfeat': torch.cat(dfeat)}
    for i in range(5):
        res[f'dW{i}'] = acc[f'{DEC}.{2 * i}.weight'].detach()
        res[f'db{i}'] = acc[f'{DEC}.{2 * i}.bias'].detach()
    return res


def elementwise_err(got, ref64):
    """(err, flat index of the worst element): err = max_i |got_i - ref64_i| / rms(ref64).  A reference that is zero
    everywhere gives err = 0 if `got` is zero too and inf otherwise; a non-finite `got` element gives inf at that element."""
    g = got.detach().double().cpu().reshape(-1)
    r = ref64.detach().double().cpu().reshape(-1)
    assert g.numel() == r.numel() and g.numel() > 0, (tuple(got.shape), tuple(ref64.shape))
    d = (g - r).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    i = int(d.argmax())
    rms = float(r.square().mean().sqrt())
    if rms == 0.0:
        return (0.0 if float(d[i]) == 0.0 else float('inf')), i
    return float(d[i]) / rms, i


def bar_for(err_ref32):
    """Ten times what the oracle's own arithmetic in fp32 misses fp64 by, floored at 64 fp32 roundings."""
    return max(BAR_FACTOR * err_ref32, BAR_FLOOR)


def check_tensor(name, got, ref64, ref32, axes, report=None):
    """Assert the elementwise bar for one tensor (`got` in the layout of `ref64`).  axes: names of the tensor's dimensions,
    used to spell out the worst element's coordinate.  report (a list) collects (name, err, err_ref32, bar) for the log."""
    assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    err, i = elementwise_err(got, ref64)
    err32, _ = elementwise_err(ref32, ref64)
    bar = bar_for(err32)
    if report is not None:
        report.append((name, err, err32, bar))
    coord = np.unravel_index(i, tuple(ref64.shape))
    where = ', '.join(f'{a}={int(c)}' for a, c in zip(axes, coord))
    g = float(got.detach().reshape(-1)[i])
    r = float(ref64.detach().reshape(-1)[i])
    assert err <= bar, (f'{name}: worst element at flat index {i} ({where}): got {g!r} ref {r!r}, err {err:.3e} > bar {bar:.3e} '
                        f'(err_ref32 {err32:.3e}; bar = max(10 * err_ref32, 64 eps_fp32))')
    return err, err32, bar
