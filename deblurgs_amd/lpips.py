"""LPIPS with the AlexNet backbone (below) and with the VGG16 backbone (further below: what metrics.py:74 reports).
AlexNet: the third number of the reference's evaluation (test.py:120:
`lpips(image, gt_image, net_type='alex')`, lpipsPyTorch/modules/{lpips,networks,utils}.py):

    z-score per channel   (x - (-.030, -.088, -.188)) / (.458, .448, .450), BEFORE the first convolution, so the
                          convolution's zero padding pads the z-scored image
    AlexNet `features`    conv 3->64 11x11 /4 pad 2, ReLU, max-pool 3x3 /2; conv 64->192 5x5 pad 2, ReLU, max-pool 3x3 /2;
                          conv 192->384, 384->256, 256->256 3x3 pad 1, each with a ReLU
    taps                  the five ReLU outputs (modules 2, 5, 8, 10, 12 counted from 1), each before its pool
    per tap               every pixel's channel vector / (sqrt(sum c^2) + 1e-10); the squared difference of the two maps;
                          the 1x1 "lin" convolution [1,C,1,1] without bias; the spatial mean
    result                the sum of the five layer values -- and, for a batch of N pairs, over the batch too: the
                          reference returns ONE [1,1,1,1] tensor (lpips.py:33-36); `lpips` keeps that, `lpips_layers`
                          and the C ABI return per-pair values

Inputs are used as they come (no rescaling to [-1, 1]); the smallest image the network accepts is 31 x 31.

The weights are the CALLER's: no file ships with this package and nothing is fetched.  `LPIPSWeights` takes the two
state dicts a user already has (torchvision's AlexNet and the published LPIPS v0.1 `alex.pth`).  fp32 device inputs run
dgs_lpips_alex (csrc/lpips.hip: an implicit-GEMM convolution on the f32 matrix cores, a max-pool and a layer-distance
kernel; no MIOpen, no host synchronisation); anything else (CPU, fp64) runs the torch expressions below.
tests/golden/lpips_golden.npz pins both paths against the reference's own module.

VGG16 (`net_type='vgg'`, networks.py:88-96): the same z-score, thirteen conv 3x3 pad 1 each with a ReLU, max-pool 2x2 /2
after convolutions 2, 4, 7 and 10; taps after convolutions 2, 4, 7, 10 (before the pool) and 13 -- torchvision's
`features` modules 4, 9, 16, 23, 30 counted from 1; the smallest image is 16 x 16.  `LPIPSVggWeights` takes torchvision's
VGG16 state dict and the published `vgg.pth`; fp32 device inputs run dgs_lpips_vgg (csrc/lpips.hip: conv3x3_kernel reads
its operands from an input halo tile in LDS).  Which backbone a call runs is the weights' `net_type`.
tests/golden/lpips_vgg_golden.npz pins both paths.

SqueezeNet 1.1 (`net_type='squeeze'`, networks.py:69-77): the same z-score, conv 3->64 3x3 /2 without padding, ReLU,
max-pool, Fire 1, Fire 2, max-pool, Fire 3, Fire 4, max-pool, Fire 5 .. 8 -- a Fire module is
cat(relu(expand1x1(s)), relu(expand3x3(s, pad 1))) with s = relu(squeeze(x)), the max-pools are 3x3 /2 with
ceil_mode=True; seven taps: the first ReLU and Fires 2, 4, 5, 6, 7, 8, each before the pool that follows it
(`features` modules 2, 5, 8, 10, 11, 12, 13 counted from 1); the smallest image is 17 x 17 and the result has eight
columns.  `LPIPSSqueezeWeights` takes torchvision's squeezenet1_1 state dict and the published `squeeze.pth`; fp32 device
inputs run dgs_lpips_squeeze (csrc/lpips.hip: fire_kernel makes a whole Fire module in one launch, the squeeze map never
leaves LDS).  tests/golden/lpips_squeeze_golden.npz pins both paths.
"""
import collections
import ctypes
import glob
import os

import torch
import torch.nn.functional as F

from . import _lib
from .raster_call import _ptr, _stream

MEAN = (-.030, -.088, -.188)                  # networks.py:41-44
STD = (.458, .448, .450)
# (Cout, Cin, kernel, stride, pad, pooled afterwards) of the five convolutions; their index in torchvision's `features`
CONVS = ((64, 3, 11, 4, 2, True), (192, 64, 5, 1, 2, True), (384, 192, 3, 1, 1, False), (256, 384, 3, 1, 1, False),
         (256, 256, 3, 1, 1, False))
FEATURE_INDEX = (0, 3, 6, 8, 10)
CHANNELS = tuple(c[0] for c in CONVS)
MIN_SIZE = 31
# VGG16: Cout of the thirteen convolutions, their index in torchvision's `features`, the tap each one feeds (or None)
VGG_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
VGG_CIN = (3,) + VGG_COUT[:-1]
VGG_FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_TAP = (None, 0, None, 1, None, None, 2, None, None, 3, None, None, 4)
VGG_CHANNELS = (64, 128, 256, 512, 512)
VGG_MIN_SIZE = 16
# SqueezeNet 1.1: (Cin, S, E) of the eight Fire modules, their index in torchvision's `features`, the tap each one feeds
# (or None), whether a ceil-mode pool follows
SQUEEZE_FIRES = ((64, 16, 64), (128, 16, 64), (128, 32, 128), (256, 32, 128), (256, 48, 192), (384, 48, 192), (384, 64, 256),
                 (512, 64, 256))
SQUEEZE_FEATURE_INDEX = (3, 4, 6, 7, 9, 10, 11, 12)
SQUEEZE_TAP = (None, 1, None, 2, 3, 4, 5, 6)
SQUEEZE_POOL = (False, True, False, True, False, False, False, False)
SQUEEZE_CHANNELS = (64, 128, 256, 384, 384, 512, 512)
SQUEEZE_MIN_SIZE = 17
FIRE_PARTS = ("squeeze", "expand1x1", "expand3x3")
MAX_TMP_BYTES = 4 << 30


def _pick(sd, names, what):
    for n in names:
        if n in sd:
            return n, sd[n]
    raise KeyError(f"LPIPS weights: {what} is missing (looked for {' / '.join(repr(n) for n in names)})")


def _as_f32(name, t, shape):
    t = torch.as_tensor(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"LPIPS weights: {name!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to(torch.float32).contiguous()


# A backbone as a layer program, the table csrc/lpips.hip walks too: per layer its kind ("conv" or "fire"), its index in
# torchvision's `features`, Cin, Cout (a Fire module: 2 E), kernel, stride, pad, the squeeze depth of a Fire module, the tap
# it feeds (or None) and the max_pool2d arguments of the pool that follows (or None)
_Layer = collections.namedtuple("_Layer", "kind index cin cout k stride pad squeeze tap pool")
_POOL_3X3, _POOL_2X2, _POOL_3X3_CEIL = {"kernel_size": 3, "stride": 2}, {"kernel_size": 2, "stride": 2}, \
    {"kernel_size": 3, "stride": 2, "ceil_mode": True}
_ALEX = tuple(_Layer("conv", idx, ci, co, k, stride, pad, None, tap, _POOL_3X3 if pool else None)
              for tap, (idx, (co, ci, k, stride, pad, pool)) in enumerate(zip(FEATURE_INDEX, CONVS)))
_VGG = tuple(_Layer("conv", idx, ci, co, 3, 1, 1, None, tap, _POOL_2X2 if tap in (0, 1, 2, 3) else None)
             for idx, ci, co, tap in zip(VGG_FEATURE_INDEX, VGG_CIN, VGG_COUT, VGG_TAP))
_SQUEEZE = (_Layer("conv", 0, 3, 64, 3, 2, 0, None, 0, _POOL_3X3_CEIL),) + tuple(
    _Layer("fire", idx, ci, 2 * e, 3, 1, 1, sq, tap, _POOL_3X3_CEIL if pool else None)
    for idx, (ci, sq, e), tap, pool in zip(SQUEEZE_FEATURE_INDEX, SQUEEZE_FIRES, SQUEEZE_TAP, SQUEEZE_POOL))


def _layer_keys(layer):
    """[(key below `features.`, shape)] of a layer's tensors, in the order the C ABI holds them."""
    if layer.kind == "conv":
        return [(f"{layer.index}.weight", (layer.cout, layer.cin, layer.k, layer.k)), (f"{layer.index}.bias", (layer.cout,))]
    sq, e = layer.squeeze, layer.cout // 2
    return [kv for part, shape in zip(FIRE_PARTS, ((sq, layer.cin, 1, 1), (e, sq, 1, 1), (e, sq, 3, 3)))
            for kv in ((f"{layer.index}.{part}.weight", shape), (f"{layer.index}.{part}.bias", shape[:1]))]


def _flat(x):
    return [x] if torch.is_tensor(x) else [t for y in x for t in _flat(y)]


def _moved(x, device):
    return x.to(device) if torch.is_tensor(x) else type(x)(_moved(y, device) for y in x)


class _Weights:
    """What the three backbones' weights share.  A subclass names its layer program, its ABI struct and the attributes
    that hold its tensors -- in the struct's order, which is a plain run of pointers."""
    net_type = min_size = _program = _abi = None
    _fields = ("conv_w", "conv_b", "lin")

    def __init__(self, conv_w, conv_b, lin):
        self.conv_w, self.conv_b, self.lin = list(conv_w), list(conv_b), list(lin)
        self._struct = None

    @classmethod
    def _from_layers(cls, layers, lin):
        return cls(*zip(*layers), lin)

    def _per_layer(self):
        """The tensors of each layer of the program: (w, bias), or a Fire module's six."""
        return list(zip(self.conv_w, self.conv_b))

    @classmethod
    def from_state_dicts(cls, features_sd, lin_sd):
        """features_sd: torchvision's state dict of the backbone (`features.{index}.{weight,bias}`, a Fire module's
        `features.{index}.{squeeze,expand1x1,expand3x3}.{weight,bias}`) or the state dict of its `.features` alone
        (`{index}. ...`).  lin_sd: the published `lin{i}.model.1.weight`, or the reference's renamed `{i}.1.weight`
        (lpipsPyTorch/modules/utils.py:22-28).  A missing key or a wrong shape raises with the key named."""
        layers = [tuple(_as_f32(*_pick(features_sd, (f"features.{key}", key), f"features.{key}"), shape)
                        for key, shape in _layer_keys(layer)) for layer in cls._program]
        channels = [layer.cout for layer in cls._program if layer.tap is not None]
        lin = [_as_f32(*_pick(lin_sd, (f"lin{i}.model.1.weight", f"{i}.1.weight"), f"lin{i}.model.1.weight"), (1, c, 1, 1))
               for i, c in enumerate(channels)]
        return cls._from_layers(layers, lin)

    @classmethod
    def load(cls, backbone_path, lin_path):
        """The two local checkpoint files (torch.load on the CPU, tensors only)."""
        return cls.from_state_dicts(torch.load(backbone_path, map_location="cpu", weights_only=True),
                                    torch.load(lin_path, map_location="cpu", weights_only=True))

    def tensors(self):
        return _flat([getattr(self, f) for f in self._fields])

    @property
    def device(self):
        return _flat(self.conv_w)[0].device

    def to(self, device):
        return type(self)(*(_moved(getattr(self, f), device) for f in self._fields))

    def struct(self):
        """The ABI struct of these tensors (they stay alive with this object)."""
        if self._struct is None:
            s = self._abi()
            slots = ctypes.cast(ctypes.pointer(s), ctypes.POINTER(ctypes.c_void_p))
            for i, t in enumerate(self.tensors()):
                slots[i] = t.data_ptr()
            self._struct = s
        return self._struct


class LPIPSWeights(_Weights):
    """The fifteen tensors of LPIPS-alex: `conv_w[i]` [Cout,Cin,k,k], `conv_b[i]` [Cout], `lin[i]` [1,C,1,1]; from
    torchvision's AlexNet state dict (`features.{0,3,6,8,10}`) and the published `alex.pth`."""
    net_type, min_size, _program, _abi = "alex", MIN_SIZE, _ALEX, _lib.DgsLpipsAlexWeights


class LPIPSVggWeights(_Weights):
    """The thirty-one tensors of LPIPS-vgg: `conv_w[i]` [Cout,Cin,3,3], `conv_b[i]` [Cout] (13 each), `lin[i]` [1,C,1,1];
    from torchvision's VGG16 state dict (`features.{0,2,5,...,28}`) and the published `vgg.pth`."""
    net_type, min_size, _program, _abi = "vgg", VGG_MIN_SIZE, _VGG, _lib.DgsLpipsVggWeights


class LPIPSSqueezeWeights(_Weights):
    """The fifty-seven tensors of LPIPS-squeeze: `conv_w` [64,3,3,3], `conv_b` [64]; `fire[i]` = (squeeze_w [S,Cin,1,1],
    squeeze_b [S], expand1_w [E,S,1,1], expand1_b [E], expand3_w [E,S,3,3], expand3_b [E]) for the eight Fire modules;
    `lin[i]` [1,C,1,1] (7); from torchvision's squeezenet1_1 state dict (`features.0`, `features.{3,4,6,7,9,10,11,12}`)
    and the published `squeeze.pth`."""
    net_type, min_size, _program, _abi = "squeeze", SQUEEZE_MIN_SIZE, _SQUEEZE, _lib.DgsLpipsSqueezeWeights
    _fields = ("conv_w", "conv_b", "fire", "lin")

    def __init__(self, conv_w, conv_b, fire, lin):
        self.conv_w, self.conv_b, self.fire, self.lin = conv_w, conv_b, [tuple(f) for f in fire], list(lin)
        self._struct = None

    @classmethod
    def _from_layers(cls, layers, lin):
        return cls(*layers[0], layers[1:], lin)

    def _per_layer(self):
        return [(self.conv_w, self.conv_b)] + self.fire



def _fire_torch(x, six):
    """A Fire module (torchvision's squeezenet.py): six = (squeeze_w, squeeze_b, expand1_w, expand1_b, expand3_w, expand3_b)
    in x's dtype on x's device."""
    s = F.relu(F.conv2d(x, six[0], six[1]))
    return torch.cat([F.relu(F.conv2d(s, six[2], six[3])), F.relu(F.conv2d(s, six[4], six[5], padding=1))], dim=1)


def _batched(x, y, min_size=MIN_SIZE):
    if x.shape != y.shape or x.dim() not in (3, 4) or x.shape[-3] != 3:
        raise ValueError(f"lpips takes two [3,H,W] or [N,3,H,W] tensors of one shape (got {tuple(x.shape)}, {tuple(y.shape)})")
    if x.dim() == 3:
        x, y = x[None], y[None]
    if x.shape[-1] < min_size or x.shape[-2] < min_size:
        raise ValueError(f"lpips needs images of at least {min_size} x {min_size} pixels (got {x.shape[-2]} x {x.shape[-1]})")
    return x, y


def _features_torch(x, w):
    """The normalised taps of x [N,3,H,W] (networks.py:53-66; five, for squeeze seven) in x's dtype on x's device."""
    t = lambda a: a.to(device=x.device, dtype=x.dtype)
    x = (x - t(torch.tensor(MEAN))[None, :, None, None]) / t(torch.tensor(STD))[None, :, None, None]
    out = []
    for layer, tensors in zip(w._program, w._per_layer()):
        tensors = [t(a) for a in tensors]
        if layer.kind == "fire":
            x = _fire_torch(x, tensors)
        else:
            x = F.relu(F.conv2d(x, tensors[0], tensors[1], stride=layer.stride, padding=layer.pad))
        if layer.tap is not None:
            out.append(x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10))
        if layer.pool is not None:
            x = F.max_pool2d(x, **layer.pool)
    return out


def _layers_torch(x, y, w):
    fx, fy = _features_torch(x, w), _features_torch(y, w)
    res = [F.conv2d((a - b) ** 2, w.lin[i].to(device=x.device, dtype=x.dtype)).mean((2, 3)) for i, (a, b) in enumerate(zip(fx, fy))]
    layers = torch.cat(res, dim=1)                                           # [N,5] (squeeze: [N,7])
    return torch.cat([layers.sum(dim=1, keepdim=True), layers], dim=1)       # [N,6] (squeeze: [N,8])


def _fused_ok(x, y):
    return (x.device.type == "cuda" and y.device == x.device and x.dtype == torch.float32 and y.dtype == torch.float32)


def lpips_layers(x, y, weights, max_tmp_bytes=MAX_TMP_BYTES):
    """[N,6] = (total, layer 1..5) per pair of x, y ([3,H,W] or [N,3,H,W]) with the backbone of `weights` (LPIPSWeights:
    alex, LPIPSVggWeights: vgg, LPIPSSqueezeWeights: squeeze, whose seven taps give [N,8]).  fp32 device inputs:
    dgs_lpips_alex / dgs_lpips_vgg / dgs_lpips_squeeze on the current stream (the weights must live on that device), no
    host synchronisation; otherwise the torch expressions in the inputs' dtype.  A batch of any backbone whose scratch
    would pass max_tmp_bytes is cut into consecutive calls: a pair's numbers do not depend on the other pairs of its
    call, so the result is the same bit for bit."""
    x, y = _batched(x, y, weights.min_size)
    if not _fused_ok(x, y):
        return _layers_torch(x, y, weights)
    if weights.device != x.device:
        raise RuntimeError(f"lpips: the weights are on {weights.device}, the images on {x.device} (use weights.to(device))")
    x, y = x.contiguous(), y.contiguous()
    L = _lib.lib()
    N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    out = torch.empty((N, len(weights.lin) + 1), dtype=torch.float32, device=x.device)
    name = "dgs_lpips_" + weights.net_type
    call, tmp_bytes = getattr(L, name), getattr(L, name + "_tmp_bytes")
    per_call = N
    while per_call > 1 and tmp_bytes(W, H, per_call) > max_tmp_bytes:
        per_call = (per_call + 1) // 2
    tmp = torch.empty(tmp_bytes(W, H, per_call), dtype=torch.uint8, device=x.device)
    st = _stream(x.device)
    for i in range(0, N, per_call):
        n = min(per_call, N - i)
        _lib.check(call(_ptr(x[i:i + n]), _ptr(y[i:i + n]), n, W, H, ctypes.byref(weights.struct()), _ptr(tmp),
                        _ptr(out[i:i + n]), st), name)
    return out


def conv2d_bias_relu(x, weight, bias, stride=1, padding=0, zscore=False):
    """relu(conv2d(x, weight, bias, stride, padding)) of fp32 device tensors through dgs_conv2d_bias_relu, the convolution
    kernel of dgs_lpips_alex on its own (x [N,Cin,H,W]; zscore: the first layer's fused z-score, Cin = 3).  No fallback."""
    if not (_fused_ok(x, weight) and _fused_ok(x, bias)) or x.dim() != 4 or weight.dim() != 4:
        raise RuntimeError("conv2d_bias_relu needs float32 tensors on one HIP device: x [N,Cin,H,W], weight [Cout,Cin,KH,KW]")
    x, weight, bias = x.contiguous(), weight.contiguous(), bias.contiguous()
    N, Cin, IH, IW = (int(v) for v in x.shape)
    Cout, _, KH, KW = (int(v) for v in weight.shape)
    if weight.shape[1] != Cin or tuple(bias.shape) != (Cout,):
        raise ValueError("conv2d_bias_relu: weight is [Cout,Cin,KH,KW] and bias [Cout]")
    OH, OW = (IH + 2 * padding - KH) // stride + 1, (IW + 2 * padding - KW) // stride + 1
    out = torch.empty((N, Cout, max(OH, 0), max(OW, 0)), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dgs_conv2d_bias_relu(_ptr(x), N, Cin, IH, IW, _ptr(weight), _ptr(bias), Cout, KH, KW, int(stride),
                                               int(padding), int(bool(zscore)), _ptr(out), _stream(x.device)),
               "dgs_conv2d_bias_relu")
    return out


def conv3x3_bias_relu(x, weight, bias, zscore=False):
    """relu(conv2d(x, weight, bias, stride 1, padding 1)), weight [Cout,Cin,3,3], through dgs_conv3x3_bias_relu, the
    halo-tile convolution kernel of dgs_lpips_vgg on its own.  No fallback."""
    if not (_fused_ok(x, weight) and _fused_ok(x, bias)) or x.dim() != 4 or weight.dim() != 4:
        raise RuntimeError("conv3x3_bias_relu needs float32 tensors on one HIP device: x [N,Cin,H,W], weight [Cout,Cin,3,3]")
    x, weight, bias = x.contiguous(), weight.contiguous(), bias.contiguous()
    N, Cin, IH, IW = (int(v) for v in x.shape)
    Cout = int(weight.shape[0])
    if tuple(weight.shape) != (Cout, Cin, 3, 3) or tuple(bias.shape) != (Cout,):
        raise ValueError("conv3x3_bias_relu: weight is [Cout,Cin,3,3] and bias [Cout]")
    out = torch.empty((N, Cout, IH, IW), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dgs_conv3x3_bias_relu(_ptr(x), N, Cin, IH, IW, _ptr(weight), _ptr(bias), Cout, int(bool(zscore)),
                                                _ptr(out), _stream(x.device)), "dgs_conv3x3_bias_relu")
    return out


def maxpool2x2(x):
    """max_pool2d(x, 2, 2) of a float32 device tensor [..., H, W] through dgs_maxpool2x2.  No fallback."""
    if not _fused_ok(x, x) or x.dim() < 2:
        raise RuntimeError("maxpool2x2 needs a float32 tensor [..., H, W] on a HIP device")
    x = x.contiguous()
    IH, IW = int(x.shape[-2]), int(x.shape[-1])
    planes = x.numel() // max(IH * IW, 1)
    out = torch.empty(tuple(x.shape[:-2]) + (IH // 2, IW // 2), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dgs_maxpool2x2(_ptr(x), planes, IH, IW, _ptr(out), _stream(x.device)), "dgs_maxpool2x2")
    return out


def fire_bias_relu(x, weights6, return_squeeze=False):
    """A Fire module, cat(relu(conv1x1(s)), relu(conv3x3(s, pad 1))) with s = relu(conv1x1(x)), through dgs_fire_bias_relu,
    the one-launch kernel of dgs_lpips_squeeze on its own.  weights6 = (squeeze_w [S,Cin,1,1], squeeze_b [S], expand1_w
    [E1,S,1,1], expand1_b [E1], expand3_w [E3,S,3,3], expand3_b [E3]), S <= 64.  return_squeeze: also the squeeze map the
    kernel computed, (out, s).  No fallback."""
    ws = tuple(weights6)
    if len(ws) != 6 or not all(_fused_ok(x, w) for w in ws) or x.dim() != 4:
        raise RuntimeError("fire_bias_relu needs float32 tensors on one HIP device: x [N,Cin,H,W] and the six Fire weights")
    x = x.contiguous()
    ws = tuple(w.contiguous() for w in ws)
    N, Cin, IH, IW = (int(v) for v in x.shape)
    S, E1, E3 = int(ws[0].shape[0]), int(ws[2].shape[0]), int(ws[4].shape[0])
    want = ((S, Cin, 1, 1), (S,), (E1, S, 1, 1), (E1,), (E3, S, 3, 3), (E3,))
    if [tuple(w.shape) for w in ws] != list(want):
        raise ValueError("fire_bias_relu: the weights are squeeze [S,Cin,1,1], [S], expand1x1 [E1,S,1,1], [E1], expand3x3 "
                         "[E3,S,3,3], [E3]")
    out = torch.empty((N, E1 + E3, IH, IW), dtype=torch.float32, device=x.device)
    sq = torch.empty((N, S, IH, IW), dtype=torch.float32, device=x.device) if return_squeeze else None
    fw = _lib.DgsFireWeights(*[w.data_ptr() for w in ws])
    _lib.check(_lib.lib().dgs_fire_bias_relu(_ptr(x), N, Cin, IH, IW, S, E1, E3, ctypes.byref(fw), _ptr(sq), _ptr(out),
                                             _stream(x.device)), "dgs_fire_bias_relu")
    return (out, sq) if return_squeeze else out


def maxpool3x3s2_ceil(x):
    """max_pool2d(x, 3, 2, ceil_mode=True) of a float32 device tensor [..., H, W] through dgs_maxpool3x3s2_ceil.  No
    fallback."""
    if not _fused_ok(x, x) or x.dim() < 2:
        raise RuntimeError("maxpool3x3s2_ceil needs a float32 tensor [..., H, W] on a HIP device")
    x = x.contiguous()
    IH, IW = int(x.shape[-2]), int(x.shape[-1])
    planes = x.numel() // max(IH * IW, 1)
    out = torch.empty(tuple(x.shape[:-2]) + (IH // 2, IW // 2), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dgs_maxpool3x3s2_ceil(_ptr(x), planes, IH, IW, _ptr(out), _stream(x.device)), "dgs_maxpool3x3s2_ceil")
    return out


def lpips(x, y, weights):
    """The reference's criterion (lpips.py:28-36): [3,H,W] or [N,3,H,W] in, ONE [1,1,1,1] tensor out -- the sum over the
    layers and over the batch."""
    return lpips_layers(x, y, weights)[:, 0].sum().reshape(1, 1, 1, 1)


# ---- the weights the drop-in `lpipsPyTorch.lpips` uses
_default = {"alex": {}, "vgg": {}, "squeeze": {}}
# per backbone: the class, torchvision's checkpoint (a glob), the LPIPS v0.1 linear layers
_FILES = {"alex": (LPIPSWeights, "alexnet-owt-*.pth", "alex.pth"), "vgg": (LPIPSVggWeights, "vgg16-*.pth", "vgg.pth"),
          "squeeze": (LPIPSSqueezeWeights, "squeezenet1_1-*.pth", "squeeze.pth")}
_BACKBONE_NAME = {"alex": "AlexNet", "vgg": "VGG16", "squeeze": "SqueezeNet 1.1"}


def set_default_weights(weights):
    """The weights `deblurgs_amd/dropin/lpipsPyTorch` evaluates with, filed under their net_type (None: forget them all)."""
    if weights is None:
        for d in _default.values():
            d.clear()
        return
    _default[weights.net_type].clear()
    _default[weights.net_type][weights.device] = weights


def default_weights(device, net_type="alex"):
    """The default weights of a backbone on `device`: those of set_default_weights, else the two files a user of
    torchvision and of the LPIPS package already has in torch.hub's checkpoint directory.  Only local files are opened;
    nothing is fetched."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    have = _default[net_type]
    if device in have:
        return have[device]
    if have:
        w = next(iter(have.values())).to(device)
    else:
        cls, backbone_glob, lin_name = _FILES[net_type]
        ckpt = os.path.join(torch.hub.get_dir(), "checkpoints")
        backbone = sorted(glob.glob(os.path.join(ckpt, backbone_glob)))
        lin = os.path.join(ckpt, lin_name)
        if not backbone or not os.path.exists(lin):
            raise FileNotFoundError(
                f"LPIPS needs two weight files and neither ships with this package: torchvision's "
                f"{_BACKBONE_NAME[net_type]} checkpoint ({backbone_glob}) and the LPIPS v0.1 linear layers "
                f"({lin_name}).  Put both into {ckpt}, or call "
                f"deblurgs_amd.lpips.set_default_weights({cls.__name__}.load(backbone_path, lin_path)).")
        w = cls.load(backbone[-1], lin).to(device)
    have[device] = w
    return w
