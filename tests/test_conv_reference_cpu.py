"""CPU (-m "not gpu"): the chunked fp64 reference of the convolution stack (oracle/conv_reference.py, used by
tests/test_gpu_conv_stack.py) equals the unchunked oracle to fp64 rounding, and its error metric sees one wrong element."""
import pytest
import torch

from oracle import conv_reference as R
from oracle import dreamer_oracle as O

FP64_BAR = 1e-12      # the chunk sums differ from the whole-batch sums by summation order only: ~1e-15 of the tensor's rms


def _inputs(oconf, frames, seed, u8):
    g = torch.Generator().manual_seed(seed)
    ch = oconf.image_channels
    raw = torch.randint(0, 256, (frames, 64, 64, ch), generator=g, dtype=torch.uint8)
    image = raw if u8 else (raw.float() / 255.0 - 0.5).permute(0, 3, 1, 2).contiguous()
    feat = torch.randn(frames, O.feature_dim(oconf), generator=g)
    dembed = torch.randn(frames, 32 * oconf.cnn_depth, generator=g)
    row_scale = 0.25 + 1.5 * torch.rand(frames, generator=g)
    return image, feat, dembed, row_scale


@pytest.mark.parametrize('depth,ch,frames,chunk,u8', [(8, 3, 11, 4, False), (8, 3, 11, 5, True), (6, 1, 7, 3, False), (8, 3, 9, 128, False)])
def test_chunked_reference_equals_unchunked(depth, ch, frames, chunk, u8):
    """Chunks of 4 and 5 do not divide 11 frames, 3 does not divide 7; 128 > 9 is the single-chunk case."""
    oconf = O.tiny_conf(cnn_depth=depth, image_channels=ch)
    params = O.make_params(oconf)
    image, feat, dembed, row_scale = _inputs(oconf, frames, 7, u8)
    x64 = R.to_frames(image, torch.float64)
    # unchunked, straight from the oracle
    p = {k: v.double().requires_grad_(True) for k, v in params.items() if 'encoder' in k or 'decoder.image' in k}
    emb = O.conv_encoder(p, x64[None])[0]
    emb.backward(dembed.double())
    enc = R.encoder_reference(params, image, dembed, chunk=chunk)
    assert R.elementwise_err(enc['embed'], emb)[0] < FP64_BAR
    for i in range(4):
        assert R.elementwise_err(enc[f'dW{i}'], p[f'{R.ENC}.{2 * i}.weight'].grad)[0] < FP64_BAR, i
        assert R.elementwise_err(enc[f'db{i}'], p[f'{R.ENC}.{2 * i}.bias'].grad)[0] < FP64_BAR, i
    f = feat.double().requires_grad_(True)
    pred = O.conv_decoder(p, f)
    loss = 0.5 * torch.square(pred - x64).sum(dim=[-1, -2, -3])
    (loss * row_scale.double() * 0.37).sum().backward()
    dec = R.decoder_reference(params, feat, image, 0.37, row_scale=row_scale, chunk=chunk)
    assert R.elementwise_err(dec['image_rec'], pred)[0] < FP64_BAR
    assert R.elementwise_err(dec['loss_image'], loss)[0] < FP64_BAR
    assert R.elementwise_err(dec['dfeat'], f.grad)[0] < FP64_BAR
    for i in range(5):
        assert R.elementwise_err(dec[f'dW{i}'], p[f'{R.DEC}.{2 * i}.weight'].grad)[0] < FP64_BAR, i
        assert R.elementwise_err(dec[f'db{i}'], p[f'{R.DEC}.{2 * i}.bias'].grad)[0] < FP64_BAR, i


def test_chunked_reference_iwae_targets():
    """tdiv = 3: prediction frame n is compared with target frame n // 3, across chunk borders (chunk 4, 9 frames)."""
    oconf = O.tiny_conf(cnn_depth=8)
    params = O.make_params(oconf)
    image, feat, _, row_scale = _inputs(oconf, 9, 3, False)
    target = image[:3]
    p = {k: v.double().requires_grad_(True) for k, v in params.items() if 'decoder.image' in k}
    f = feat.double().requires_grad_(True)
    pred = O.conv_decoder(p, f)
    loss = 0.5 * torch.square(pred - target.double().repeat_interleave(3, 0)).sum(dim=[-1, -2, -3])
    (loss * row_scale.double() * 2.0).sum().backward()
    dec = R.decoder_reference(params, feat, target, 2.0, row_scale=row_scale, tdiv=3, chunk=4)
    assert R.elementwise_err(dec['loss_image'], loss)[0] < FP64_BAR
    assert R.elementwise_err(dec['dfeat'], f.grad)[0] < FP64_BAR
    assert R.elementwise_err(dec['dW4'], p[f'{R.DEC}.8.weight'].grad)[0] < FP64_BAR


def test_metric_sees_one_wrong_element_and_names_it():
    ref = torch.randn(3, 5, 7, 2, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    ref32 = ref.float()
    got = ref.float().clone()
    R.check_tensor('t', got, ref, ref32, ('a', 'b', 'c', 'd'))
    got[1, 4, 6, 1] += 1.0
    err, i = R.elementwise_err(got, ref)
    assert 0.5 < err < 2.0 and i == ((1 * 5 + 4) * 7 + 6) * 2 + 1
    with pytest.raises(AssertionError, match=r't: worst element at flat index 139 \(a=1, b=4, c=6, d=1\)'):
        R.check_tensor('t', got, ref, ref32, ('a', 'b', 'c', 'd'))
    got[1, 4, 6, 1] = float('nan')
    assert R.elementwise_err(got, ref) == (float('inf'), 139)
    assert R.bar_for(0.0) == R.BAR_FLOOR == 64 * 2.0 ** -23 and R.bar_for(1e-5) == pytest.approx(1e-4)
