"""-m gpu: the gather-form transposed convolutions with their zero-border k-tiles skipped (dm_convt_kskip_enable, csrc/conv.hip:
rows ordered (chunk of 128 frames, yy, xx, frame in chunk), a k-tile list per 128 rows) against the same library with the switch
off (rows ordered (frame, yy, xx), every k-tile) and against the fp64 CPU oracle.

The three products of this form - decoder layer 3 forward, the encoder's layer-3 and layer-2 data gradients - are reached through
dm_conv_decoder_mse_fwd and dm_conv_encoder_fwd + _bwd, called through the C-ABI as tests/test_gpu_conv_stack.py calls them.

  cnn_depth 16: the decoder layer has cin = 32, one 32-k tile per tap;  cnn_depth 24: cin = 48, a tile spans two taps.
  frames 1, 3 (less than a chunk: every block of rows straddles class pixels), 130 (a chunk and a short one of 2 frames),
  257 (two chunks and one frame).
  dm_gemm_dma_enable(0) and (2): the register-staged loop and the LDS-DMA loop both walk a list at every shape.

Checked per case:
  * switch on against switch off: every output and every gradient equal under `==` (the terms left out are 0 * w, the terms
    kept are added in the same order);
  * switch on against the fp64 reference of oracle/conv_reference.py, every element, with that file's metric and bar
    (err = max |got - ref64| / rms(ref64) <= max(10 * err of the same oracle in fp32, 64 eps)).
The workspace is exactly dm_workspace_bytes, filled with NaNs before each call, between two canary regions: a list entry read
before it is written, or a list that does not fit the workspace, shows up as a non-finite result or a damaged canary.
One reference per (depth, frames), shared by the two loops.
"""
import ctypes

import pytest
import torch

from oracle import conv_reference as R
from oracle import dreamer_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 23
GUARD = 4096
CANARY = 0x7FC5A5A5          # a quiet NaN with a payload, as int32
DEPTHS = (16, 24)
FRAMES = (1, 3, 130, 257)

_MODELS = {}
_REFS = {}


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


def _reference(depth, frames):
    """Inputs and the fp64 / fp32 CPU references, computed once per (depth, frames) and never modified."""
    key = (depth, frames)
    if key not in _REFS:
        oconf, params, _ = _model(depth)
        g = torch.Generator().manual_seed(SEED * 1000003 + 1000 * depth + frames)
        raw = torch.randint(0, 256, (frames, 64, 64, 3), generator=g, dtype=torch.uint8)
        inp = dict(raw=raw, image=(raw.float() / 255.0 - 0.5).permute(0, 3, 1, 2).contiguous(),
                   feat=torch.randn(frames, O.feature_dim(oconf), generator=g),
                   dembed=torch.randn(frames, 32 * depth, generator=g))
        ref = dict(inp=inp)
        for tag, dt in (('64', torch.float64), ('32', torch.float32)):
            ref['enc' + tag] = R.encoder_reference(params, raw, inp['dembed'], dtype=dt)
            ref['dec' + tag] = R.decoder_reference(params, inp['feat'], raw, 1.0 / frames, dtype=dt)
        _REFS[key] = ref
    return _REFS[key]


class _Buf:
    def __init__(self, numel, book):
        self.numel = int(numel)
        self.raw = torch.full((self.numel + 2 * GUARD,), CANARY, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.numel].view(torch.float32)
        book.append(self)

    def intact(self):
        return bool((self.raw[:GUARD] == CANARY).all()) and bool((self.raw[GUARD + self.numel:] == CANARY).all())


def _run(H, model, frames, inp):
    """dm_conv_encoder_fwd + _bwd and dm_conv_decoder_mse_fwd; every output on the CPU."""
    shp = model.wm.shape(1, frames, 1)
    book = []
    nbytes = H.workspace_bytes(shp)
    ws = _Buf(nbytes // 4, book)
    ws_p = ctypes.c_void_p(ws.t.data_ptr())
    enc = model.wm.encoder.encoder_image
    E = enc.out_dim
    acts = _Buf(int(H.lib().dm_conv_encoder_acts_floats(ctypes.byref(shp))), book)
    embed = _Buf(frames * E, book)
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
    out = {'embed': embed.t.view(frames, E).cpu()}
    for i, m in enumerate(enc.convs()):
        out[f'enc dW{i}'] = gw[i].t.view_as(m.weight).cpu()
        out[f'enc db{i}'] = gb[i].t.view_as(m.bias).cpu()

    dl = model.wm.decoder.image.layers()
    dacts = _Buf(int(H.lib().dm_conv_decoder_acts_floats(ctypes.byref(shp))), book)
    loss = _Buf(frames, book)
    rec = _Buf(frames * 3 * 4096, book)
    feat, target = inp['feat'].to(DEV), inp['image'].to(DEV)
    dec_p = H.conv_struct([m.weight for m in dl], [m.bias for m in dl])
    ws.raw.fill_(CANARY)
    H.call('dm_conv_decoder_mse_fwd', ctypes.byref(shp), H.fptr(feat), feat.shape[1], H.ptr(target), ctypes.byref(dec_p),
           H.fptr(dacts.t), H.fptr(loss.t), H.fptr(rec.t), ws_p, nbytes, H.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in book), f'out-of-bounds write at {frames} frames'
    off = int(H.lib().dm_conv_decoder_pred_offset(ctypes.byref(shp)))
    out['image_rec'] = rec.t.view(frames, 3, 64, 64).cpu()
    out['loss_image'] = loss.t.cpu()
    out['pred_nhwc'] = dacts.t[off:off + frames * 4096 * 3].view(frames, 64, 64, 3).cpu()
    return out


@pytest.mark.parametrize('dma', [0, 2])
@pytest.mark.parametrize('frames', FRAMES)
@pytest.mark.parametrize('depth', DEPTHS)
def test_kskip_equals_full_walk_and_matches_fp64(hip, depth, frames, dma):
    _, _, model = _model(depth)
    ref = _reference(depth, frames)
    lib = hip.lib()
    assert lib.dm_convt_kskip_enable(-1) == 1, 'the k-tile lists are on by default'
    dma_before = lib.dm_gemm_dma_enable(-1)
    lib.dm_gemm_dma_enable(dma)
    try:
        on = _run(hip, model, frames, ref['inp'])
        assert lib.dm_convt_kskip_enable(0) == 0
        off = _run(hip, model, frames, ref['inp'])
    finally:
        lib.dm_convt_kskip_enable(1)
        lib.dm_gemm_dma_enable(dma_before)
    differ = [k for k in on if not bool((on[k] == off[k]).all())]
    assert not differ, f'depth {depth} frames {frames} dma {dma}: {differ} differ between the listed and the full k walk'

    e64, e32, d64, d32 = ref['enc64'], ref['enc32'], ref['dec64'], ref['dec32']
    checks = [('encoder embed', on['embed'], e64['embed'], e32['embed'], ('frame', 'feature(c,y,x)'))]
    for i in range(4):
        checks.append((f'encoder dW{i}', on[f'enc dW{i}'], e64[f'dW{i}'], e32[f'dW{i}'], ('out', 'in', 'ky', 'kx')))
        checks.append((f'encoder db{i}', on[f'enc db{i}'], e64[f'db{i}'], e32[f'db{i}'], ('out',)))
    checks += [('decoder image_rec', on['image_rec'], d64['image_rec'], d32['image_rec'], ('frame', 'channel', 'y', 'x')),
               ('decoder pred (acts)', on['pred_nhwc'], d64['image_rec'].permute(0, 2, 3, 1), d32['image_rec'].permute(0, 2, 3, 1),
                ('frame', 'y', 'x', 'channel')),
               ('decoder loss_image', on['loss_image'], d64['loss_image'], d32['loss_image'], ('frame',))]
    report, failures = [], []
    for name, got, r64, r32, axes in checks:
        try:
            R.check_tensor(name, got, r64, r32, axes, report)
        except AssertionError as e:
            failures.append(str(e))
    print(f'\n[depth {depth} frames {frames} dma {dma}]')
    for name, err, err32, bar in report:
        print(f'  {name:<22} err {err:.3e}  err_ref32 {err32:.3e}  bar {bar:.3e}')
    assert not failures, ' | '.join(failures)
