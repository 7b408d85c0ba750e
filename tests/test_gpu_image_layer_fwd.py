"""-m gpu: the decoder image layer's forward with one patch read for all four parity classes (dm_dec_l4_fwd_shared_enable,
csrc/conv_direct.hip: the (9 d) -> 12 product on v_mfma_f32_16x16x4_f32, weights in LDS) against the same library with the switch
off (one class per wave on packed FMAs) and against the fp64 CPU oracle; and the encoder's backward, whose layer-2 data gradient
now clears only the unreached last row / column of its 31 x 31 image (convt_border_zero_kernel, csrc/conv.hip) instead of the
whole buffer.

Both are reached through the C-ABI as tests/test_gpu_convt_kskip.py reaches them: the workspace is exactly dm_workspace_bytes,
filled with NaNs before each call, between two canary regions.

Image layer, cnn_depth 8 (two channel quads per tap), 48 (the workload's depth) and 64 (the largest register and LDS footprint
the kernel admits: dynamic LDS above 64 KB), frames 1 and 3; and 65 frames at depths 8 and 48: 520 tiles of (frame, 4 class
rows) for the kernel's 512 workgroups, so that eight of them walk on to a second tile through the register prefetch:
  * switch on against switch off: pred_nhwc, loss_image and image_rec equal under `==` - per output element both kernels run the
    same chain: from the bias, taps ab = 0 .. 8 ascending, input channels ascending, one fused multiply-add per term;
  * switch on against oracle/conv_reference.decoder_reference in fp64, every element (image rows / columns 0-3 and 60-63, where
    taps fall outside the input, included), with that file's metric and bar
    (err = max |got - ref64| / rms(ref64) <= max(10 * err of the same oracle in fp32, 64 eps)).
Encoder, cnn_depth 16, frames 1 and 3: dW0..3 and db0..3 finite and within the same bar of encoder_reference - a border left
uncleared in the NaN-filled workspace reaches dW0 / db0 through the layer-1 weight gradient and bias sum.
"""
import ctypes

import pytest
import torch

from oracle import conv_reference as R
from oracle import dreamer_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 29
GUARD = 4096
CANARY = 0x7FC5A5A5          # a quiet NaN with a payload, as int32

_MODELS = {}


def _model(depth):
    if depth not in _MODELS:
        from pydreamer_amd import config
        from pydreamer_amd.models import Dreamer
        oconf = O.tiny_conf(cnn_depth=depth, image_channels=3)
        params = O.make_params(oconf)
        model = Dreamer(config.load_config('defaults', 'atari', **{k: getattr(oconf, k) for k in vars(oconf)}))
        model.load_state_dict(params, strict=True)
        _MODELS[depth] = (oconf, params, model.to(DEV))
    return _MODELS[depth]


def _inputs(depth, frames):
    oconf, _, _ = _model(depth)
    g = torch.Generator().manual_seed(SEED * 1000003 + 1000 * depth + frames)
    raw = torch.randint(0, 256, (frames, 64, 64, 3), generator=g, dtype=torch.uint8)
    return dict(raw=raw, image=(raw.float() / 255.0 - 0.5).permute(0, 3, 1, 2).contiguous(),
                feat=torch.randn(frames, O.feature_dim(oconf), generator=g),
                dembed=torch.randn(frames, 32 * depth, generator=g))


class _Buf:
    def __init__(self, numel, book):
        self.numel = int(numel)
        self.raw = torch.full((self.numel + 2 * GUARD,), CANARY, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.numel].view(torch.float32)
        book.append(self)

    def intact(self):
        return bool((self.raw[:GUARD] == CANARY).all()) and bool((self.raw[GUARD + self.numel:] == CANARY).all())


def _run_decoder(H, model, frames, inp):
    shp = model.wm.shape(1, frames, 1)
    book = []
    nbytes = H.workspace_bytes(shp)
    ws = _Buf(nbytes // 4, book)
    dl = model.wm.decoder.image.layers()
    dacts = _Buf(int(H.lib().dm_conv_decoder_acts_floats(ctypes.byref(shp))), book)
    loss = _Buf(frames, book)
    rec = _Buf(frames * 3 * 4096, book)
    feat, target = inp['feat'].to(DEV), inp['image'].to(DEV)
    dec_p = H.conv_struct([m.weight for m in dl], [m.bias for m in dl])
    H.call('dm_conv_decoder_mse_fwd', ctypes.byref(shp), H.fptr(feat), feat.shape[1], H.ptr(target), ctypes.byref(dec_p),
           H.fptr(dacts.t), H.fptr(loss.t), H.fptr(rec.t), ctypes.c_void_p(ws.t.data_ptr()), nbytes, H.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in book), f'out-of-bounds write at {frames} frames'
    off = int(H.lib().dm_conv_decoder_pred_offset(ctypes.byref(shp)))
    return {'image_rec': rec.t.view(frames, 3, 64, 64).cpu(), 'loss_image': loss.t.cpu(),
            'pred_nhwc': dacts.t[off:off + frames * 4096 * 3].view(frames, 64, 64, 3).cpu()}


def _run_encoder(H, model, frames, inp):
    shp = model.wm.shape(1, frames, 1)
    book = []
    nbytes = H.workspace_bytes(shp)
    ws = _Buf(nbytes // 4, book)
    ws_p = ctypes.c_void_p(ws.t.data_ptr())
    enc = model.wm.encoder.encoder_image
    acts = _Buf(int(H.lib().dm_conv_encoder_acts_floats(ctypes.byref(shp))), book)
    embed = _Buf(frames * enc.out_dim, book)
    gw = [_Buf(m.weight.numel(), book) for m in enc.convs()]
    gb = [_Buf(m.bias.numel(), book) for m in enc.convs()]
    image, dembed = inp['image'].to(DEV), inp['dembed'].to(DEV)
    enc_p = H.conv_struct([m.weight for m in enc.convs()], [m.bias for m in enc.convs()])
    enc_g = H.conv_struct([g.t for g in gw], [g.t for g in gb], cls=H.dm_conv_grads)
    H.call('dm_conv_encoder_fwd', ctypes.byref(shp), H.ptr(image), ctypes.byref(enc_p), H.fptr(acts.t), H.fptr(embed.t), ws_p, nbytes,
           H.stream())
    ws.raw.fill_(CANARY)
    H.call('dm_conv_encoder_bwd', ctypes.byref(shp), H.ptr(image), ctypes.byref(enc_p), H.fptr(acts.t), H.fptr(dembed),
           ctypes.byref(enc_g), ws_p, nbytes, H.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in book), f'out-of-bounds write at {frames} frames'
    out = {}
    for i, m in enumerate(enc.convs()):
        out[f'dW{i}'] = gw[i].t.view_as(m.weight).cpu()
        out[f'db{i}'] = gb[i].t.view_as(m.bias).cpu()
    return out


def _check(tag, checks):
    report, failures = [], []
    for name, got, r64, r32, axes in checks:
        try:
            R.check_tensor(name, got, r64, r32, axes, report)
        except AssertionError as e:
            failures.append(str(e))
    print(f'\n[{tag}]')
    for name, err, err32, bar in report:
        print(f'  {name:<22} err {err:.3e}  err_ref32 {err32:.3e}  bar {bar:.3e}')
    assert not failures, ' | '.join(failures)


@pytest.mark.parametrize('depth,frames', [(8, 1), (8, 3), (48, 1), (48, 3), (64, 1), (64, 3), (8, 65), (48, 65)])
def test_shared_patch_forward_equals_per_class_and_matches_fp64(hip, depth, frames):
    _, params, model = _model(depth)
    inp = _inputs(depth, frames)
    lib = hip.lib()
    assert lib.dm_dec_l4_fwd_shared_enable(-1) == 1, 'the shared-patch forward is on by default'
    try:
        on = _run_decoder(hip, model, frames, inp)
        assert lib.dm_dec_l4_fwd_shared_enable(0) == 0
        off = _run_decoder(hip, model, frames, inp)
    finally:
        lib.dm_dec_l4_fwd_shared_enable(1)
    for k in on:
        assert bool(torch.isfinite(on[k]).all()), f'depth {depth} frames {frames}: {k} is not finite'
    differ = [f'{k} ({int((on[k] != off[k]).sum())} elements)' for k in on if not bool((on[k] == off[k]).all())]
    assert not differ, f'depth {depth} frames {frames}: {differ} differ between the shared-patch and the per-class forward'

    d64 = R.decoder_reference(params, inp['feat'], inp['raw'], 1.0 / frames, dtype=torch.float64)
    d32 = R.decoder_reference(params, inp['feat'], inp['raw'], 1.0 / frames, dtype=torch.float32)
    _check(f'depth {depth} frames {frames}',
           [('decoder image_rec', on['image_rec'], d64['image_rec'], d32['image_rec'], ('frame', 'channel', 'y', 'x')),
            ('decoder pred (acts)', on['pred_nhwc'], d64['image_rec'].permute(0, 2, 3, 1), d32['image_rec'].permute(0, 2, 3, 1),
             ('frame', 'y', 'x', 'channel')),
            ('decoder loss_image', on['loss_image'], d64['loss_image'], d32['loss_image'], ('frame',))])


@pytest.mark.parametrize('frames', [1, 3])
def test_encoder_backward_from_nan_workspace(hip, frames):
    depth = 16
    _, params, model = _model(depth)
    inp = _inputs(depth, frames)
    got = _run_encoder(hip, model, frames, inp)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f'frames {frames}: encoder {k} is not finite (a gradient border left uncleared?)'
    e64 = R.encoder_reference(params, inp['raw'], inp['dembed'], dtype=torch.float64)
    e32 = R.encoder_reference(params, inp['raw'], inp['dembed'], dtype=torch.float32)
    checks = []
    for i in range(4):
        checks.append((f'encoder dW{i}', got[f'dW{i}'], e64[f'dW{i}'], e32[f'dW{i}'], ('out', 'in', 'ky', 'kx')))
        checks.append((f'encoder db{i}', got[f'db{i}'], e64[f'db{i}'], e32[f'db{i}'], ('out',)))
    _check(f'encoder depth {depth} frames {frames}', checks)
