"""Which form every layer of the convolution stack takes, per (cnn_depth, image channels): the table tests/test_conv_plan_cpu.py
holds against dm_conv_plan_query (the plans csrc/conv.hip carries out).  Written out by hand from the rules below - not computed
by the library - for every (depth, channels) of tests/test_gpu_conv_stack.py's CASES and the depths of
tests/test_gpu_convt_kskip.py, with every switch at its default and fp32 operands.

Geometry: encoder extents 64 -> 31 -> 14 -> 6 -> 2 (k 4, stride 2), channels ch -> d -> 2d -> 4d -> 8d; decoder extents
1 -> 5 -> 13 -> 30 -> 64 (k 5, 5, 6, 6), channels 32d -> 4d -> 2d -> d -> ch.  The gather form (convt_gather_ok) wants an even
kernel, input channels in fours, at least 16 output channels, (Hc / hs)^2 <= 1.4 and an output under 2^31 elements:
  encoder data gradient out of layer 3 (hs 2): never;  out of layer 2 (hs 6, 4d -> 2d): d >= 8;  out of layer 1 (hs 14,
  2d -> d): d >= 16 and even;  decoder layer 3 (hs 13, 2d -> d): d >= 16 and even;  decoder layers 1, 2: odd kernel;  decoder
  layer 4: ch < 16 output channels.
The direct kernels (encoder layer 0 both ways, decoder layer 4 both ways) want 3 channels and d in {8, 16, 32, 48, 64}.
Decoder backward: output channels that are no multiple of 4 are padded (ch 3 or 1 -> 4; d = 6 -> 8 at layer 3), and a layer whose
input gradient feeds such a padded layer writes it at the padded pitch (layer 4 at d = 6).
"""
import collections
import ctypes

# dm_conv_plan_query: form codes, bit values (out[l] = form | bits << 8), `which`
FORMS = ('direct', 'direct+planes', 'patch', 'implicit', 'gather', 'column', 'one_pixel')
BITS = {'hpath': 1, 'padded': 2, 'repitch': 4}
ENC_FWD, ENC_BWD, DEC_FWD, DEC_BWD = range(4)

# enc_fwd / enc_bwd: layers 0..3 (enc_bwd: layer 0's weight gradient, then the data gradient out of layers 1, 2, 3);
# dec_fwd / dec_bwd: layers 1..4.  'form' or 'form+bit+bit'.
Case = collections.namedtuple('Case', 'depth ch frames enc_fwd enc_bwd dec_fwd dec_bwd')
I3 = ('implicit',) * 3
CASES = [
    Case(48, 3, (2500, 1536, 1, 511, 512, 513, 1025, 67, 131),
         ('direct',) + I3, ('direct', 'gather', 'gather', 'column'),
         ('one_pixel', 'column', 'gather', 'direct'), I3 + ('direct+padded',)),
    Case(8, 3, (131,),
         ('direct',) + I3, ('direct', 'column', 'gather', 'column'),
         ('one_pixel', 'column', 'column', 'direct'), I3 + ('direct+padded',)),
    Case(16, 3, (131, 1, 3, 130, 257),
         ('direct',) + I3, ('direct', 'gather', 'gather', 'column'),
         ('one_pixel', 'column', 'gather', 'direct'), I3 + ('direct+padded',)),
    Case(32, 3, (131, 513),
         ('direct',) + I3, ('direct', 'gather', 'gather', 'column'),
         ('one_pixel', 'column', 'gather', 'direct'), I3 + ('direct+padded',)),
    Case(64, 3, (131,),
         ('direct',) + I3, ('direct', 'gather', 'gather', 'column'),
         ('one_pixel', 'column', 'gather', 'direct'), I3 + ('direct+padded',)),
    Case(24, 3, (131, 1, 3, 130, 257),
         ('patch',) + I3, ('patch', 'gather', 'gather', 'column'),
         ('one_pixel', 'column', 'gather', 'column'), I3 + ('implicit+padded',)),
    Case(12, 3, (131,),
         ('patch',) + I3, ('patch', 'column', 'gather', 'column'),
         ('one_pixel', 'column', 'column', 'column'), I3 + ('implicit+padded',)),
    Case(6, 3, (131,),
         ('patch',) + I3, ('patch', 'column', 'column', 'column'),
         ('one_pixel', 'column', 'column', 'column'), ('implicit', 'implicit', 'implicit+padded', 'implicit+padded+repitch')),
    Case(48, 1, (131,),
         ('patch',) + I3, ('patch', 'gather', 'gather', 'column'),
         ('one_pixel', 'column', 'gather', 'column'), I3 + ('implicit+padded',)),
    Case(8, 1, (131,),
         ('patch',) + I3, ('patch', 'column', 'gather', 'column'),
         ('one_pixel', 'column', 'column', 'column'), I3 + ('implicit+padded',)),
]
BY_KEY = {(c.depth, c.ch): c for c in CASES}
DIRECT_DEPTHS = (8, 16, 32, 48, 64)


def rule(depth, ch):
    """The module docstring's rules -> (enc_fwd, enc_bwd, dec_fwd, dec_bwd), to hold the hand-written rows against."""
    direct = ch == 3 and depth in DIRECT_DEPTHS
    l0 = 'direct' if direct else 'patch'
    g2 = 'gather' if depth >= 8 else 'column'
    g1 = 'gather' if depth >= 16 and depth % 2 == 0 else 'column'
    cout = (None, 4 * depth, 2 * depth, depth, ch)
    dec_bwd = []
    for l in (1, 2, 3, 4):
        form = 'direct' if direct and l == 4 else 'implicit'
        padded = '+padded' if cout[l] % 4 else ''
        repitch = '+repitch' if form == 'implicit' and l >= 2 and cout[l - 1] % 4 else ''
        dec_bwd.append(form + padded + repitch)
    return ((l0,) + I3, (l0, g1, g2, 'column'), ('one_pixel', 'column', g1, 'direct' if direct else 'column'), tuple(dec_bwd))


def code(text):
    """'implicit+padded' -> the value dm_conv_plan_query reports for that layer"""
    form, *bits = text.split('+')
    if bits and bits[0] == 'planes':
        form, bits = 'direct+planes', bits[1:]
    return FORMS.index(form) | sum(BITS[b] for b in bits) << 8


def shape(hip, depth, ch, frames, flags=0, **over):
    f = dict(T=1, B=frames, I=1, H=15, D=200, Hd=200, S=8, C=8, E=32 * depth, A=4, mlp_hidden=64, mlp_layers=2, cnn_depth=depth,
             img=64, img_ch=ch, flags=flags)
    f.update(over)
    return hip.make_shape(**f)


def query(hip, which, shp, planes=0):
    """dm_conv_plan_query -> (return code, the layer codes that exist, kskip, need in floats)"""
    out = (ctypes.c_int32 * 8)(*([-7] * 8))
    need = ctypes.c_size_t(0)
    rc = hip.lib().dm_conv_plan_query(which, ctypes.byref(shp), planes, out, ctypes.byref(need))
    return rc, tuple(v for v in out[:5] if v >= 0), int(out[5]), int(need.value)
