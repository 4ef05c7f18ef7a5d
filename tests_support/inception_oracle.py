"""Restatement of the FID Inception-v3 trunk (pytorch-fid's `InceptionV3([3])`, vendored by the reference at
evaluations/utils/inception.py) with torch.nn.functional only: no torchvision, no module classes, any float dtype.

The wiring is torchvision's Inception3 (stem, InceptionA x3, InceptionB, InceptionC x4, InceptionD, InceptionE x2) with the FID
patches: the pool branch of every A, C and of the first E block is a 3x3 average pool that does not count padding, the pool branch
of the second E block is a 3x3 MAX pool.  A basic conv is conv2d without bias, batch norm with running statistics (eps 1e-3), ReLU.

The trunk is written ONCE, as `walk(ops, x)`, over a small interface (`conv`, `maxpool`, `avgpool`, `cat`, `mean`), and run with
two implementations of it: `TensorOps` computes, `ShapeOps` only tracks (channels, side) and records every conv -- the source of
the parameter table, the parameter count and the FLOP count.
"""
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
TRUNK_PARAMETERS = 21_785_568          # learnable parameters (conv weights, norm gains and biases) of the trunk below
AUX_AND_FC_PARAMETERS = 3_326_696 + 2_049_000      # AuxLogits + fc at 1000 classes: with the trunk, torchvision's 27 161 264


def _block_a(o, p, x, pool_features):
    b1 = o.conv(p + ".branch1x1", x, 64)
    b5 = o.conv(p + ".branch5x5_2", o.conv(p + ".branch5x5_1", x, 48), 64, k=5, pad=2)
    b3 = o.conv(p + ".branch3x3dbl_1", x, 64)
    b3 = o.conv(p + ".branch3x3dbl_2", b3, 96, k=3, pad=1)
    b3 = o.conv(p + ".branch3x3dbl_3", b3, 96, k=3, pad=1)
    bp = o.conv(p + ".branch_pool", o.avgpool(x), pool_features)
    return o.cat([b1, b5, b3, bp])


def _block_b(o, p, x):
    b3 = o.conv(p + ".branch3x3", x, 384, k=3, stride=2)
    bd = o.conv(p + ".branch3x3dbl_1", x, 64)
    bd = o.conv(p + ".branch3x3dbl_2", bd, 96, k=3, pad=1)
    bd = o.conv(p + ".branch3x3dbl_3", bd, 96, k=3, stride=2)
    return o.cat([b3, bd, o.maxpool(x, stride=2, pad=0)])


def _block_c(o, p, x, c7):
    row, col = dict(k=(1, 7), pad=(0, 3)), dict(k=(7, 1), pad=(3, 0))
    b1 = o.conv(p + ".branch1x1", x, 192)
    b7 = o.conv(p + ".branch7x7_1", x, c7)
    b7 = o.conv(p + ".branch7x7_2", b7, c7, **row)
    b7 = o.conv(p + ".branch7x7_3", b7, 192, **col)
    bd = o.conv(p + ".branch7x7dbl_1", x, c7)
    bd = o.conv(p + ".branch7x7dbl_2", bd, c7, **col)
    bd = o.conv(p + ".branch7x7dbl_3", bd, c7, **row)
    bd = o.conv(p + ".branch7x7dbl_4", bd, c7, **col)
    bd = o.conv(p + ".branch7x7dbl_5", bd, 192, **row)
    bp = o.conv(p + ".branch_pool", o.avgpool(x), 192)
    return o.cat([b1, b7, bd, bp])


def _block_d(o, p, x):
    b3 = o.conv(p + ".branch3x3_2", o.conv(p + ".branch3x3_1", x, 192), 320, k=3, stride=2)
    b7 = o.conv(p + ".branch7x7x3_1", x, 192)
    b7 = o.conv(p + ".branch7x7x3_2", b7, 192, k=(1, 7), pad=(0, 3))
    b7 = o.conv(p + ".branch7x7x3_3", b7, 192, k=(7, 1), pad=(3, 0))
    b7 = o.conv(p + ".branch7x7x3_4", b7, 192, k=3, stride=2)
    return o.cat([b3, b7, o.maxpool(x, stride=2, pad=0)])


def _block_e(o, p, x, max_pool):
    row, col = dict(k=(1, 3), pad=(0, 1)), dict(k=(3, 1), pad=(1, 0))
    b1 = o.conv(p + ".branch1x1", x, 320)
    b3 = o.conv(p + ".branch3x3_1", x, 384)
    b3 = o.cat([o.conv(p + ".branch3x3_2a", b3, 384, **row), o.conv(p + ".branch3x3_2b", b3, 384, **col)])
    bd = o.conv(p + ".branch3x3dbl_1", x, 448)
    bd = o.conv(p + ".branch3x3dbl_2", bd, 384, k=3, pad=1)
    bd = o.cat([o.conv(p + ".branch3x3dbl_3a", bd, 384, **row), o.conv(p + ".branch3x3dbl_3b", bd, 384, **col)])
    pooled = o.maxpool(x, stride=1, pad=1) if max_pool else o.avgpool(x)
    return o.cat([b1, b3, bd, o.conv(p + ".branch_pool", pooled, 192)])


def walk(o, x):
    """The trunk from the (already resized and scaled) input to the pooled 2048 features."""
    x = o.conv("Conv2d_1a_3x3", x, 32, k=3, stride=2)
    x = o.conv("Conv2d_2a_3x3", x, 32, k=3)
    x = o.conv("Conv2d_2b_3x3", x, 64, k=3, pad=1)
    x = o.maxpool(x, stride=2, pad=0)
    x = o.conv("Conv2d_3b_1x1", x, 80)
    x = o.conv("Conv2d_4a_3x3", x, 192, k=3)
    x = o.maxpool(x, stride=2, pad=0)
    for name, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
        x = _block_a(o, name, x, pf)
    x = _block_b(o, "Mixed_6a", x)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        x = _block_c(o, name, x, c7)
    x = _block_d(o, "Mixed_7a", x)
    x = _block_e(o, "Mixed_7b", x, max_pool=False)
    x = _block_e(o, "Mixed_7c", x, max_pool=True)
    return o.mean(x)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class TensorOps:
    def __init__(self, sd, dtype):
        self.sd, self.dtype = sd, dtype

    def _p(self, key):
        return self.sd[key].detach().to(self.dtype)

    def conv(self, name, x, cout, k=1, stride=1, pad=0):
        w = self._p(name + ".conv.weight")
        assert w.shape == (cout, x.shape[1]) + _pair(k), (name, tuple(w.shape))
        y = F.conv2d(x, w, None, stride=stride, padding=_pair(pad))
        y = F.batch_norm(y, self._p(name + ".bn.running_mean"), self._p(name + ".bn.running_var"), self._p(name + ".bn.weight"),
                         self._p(name + ".bn.bias"), training=False, eps=BN_EPS)
        return F.relu(y)

    def maxpool(self, x, stride, pad):
        return F.max_pool2d(x, 3, stride=stride, padding=pad)

    def avgpool(self, x):
        return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)

    def cat(self, xs):
        return torch.cat(xs, 1)

    def mean(self, x):
        return x.mean((2, 3))


class ShapeOps:
    """x is (channels, side); records (name, cin, cout, (kh, kw), stride, (ph, pw), output side) per conv."""

    def __init__(self):
        self.convs = []

    def conv(self, name, x, cout, k=1, stride=1, pad=0):
        (kh, kw), (ph, pw) = _pair(k), _pair(pad)
        so = (x[1] + 2 * ph - kh) // stride + 1
        assert so == (x[1] + 2 * pw - kw) // stride + 1 and so >= 1, name
        self.convs.append((name, x[0], cout, (kh, kw), stride, (ph, pw), so))
        return cout, so

    def maxpool(self, x, stride, pad):
        return x[0], (x[1] + 2 * pad - 3) // stride + 1

    def avgpool(self, x):
        return x

    def cat(self, xs):
        assert len({s for _, s in xs}) == 1
        return sum(c for c, _ in xs), xs[0][1]

    def mean(self, x):
        return x[0], 1


def conv_table(side: int = 299):
    """[(name, cin, cout, (kh, kw), stride, (ph, pw), output side)] of the 94 convs, in execution order, for a side x side input."""
    o = ShapeOps()
    assert walk(o, (3, side)) == (2048, 1)
    return o.convs


def state_dict_shapes() -> dict:
    shapes = {}
    for name, cin, cout, k, _, _, _ in conv_table():
        shapes[name + ".conv.weight"] = (cout, cin) + k
        for v in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{v}"] = (cout,)
    return shapes


def parameter_count() -> int:
    """Learnable parameters: conv weights, norm gains and biases (running statistics are buffers)."""
    return sum(cout * cin * k[0] * k[1] + 2 * cout for _, cin, cout, k, _, _, _ in conv_table())


def flops(side: int, batch: int = 1) -> float:
    """2 x multiply-adds of every conv at this input side."""
    return float(sum(2 * batch * so * so * cout * cin * k[0] * k[1] for _, cin, cout, k, _, _, so in conv_table(side)))


def forward(sd, x, resize_input=True, normalize_input=True, dtype=torch.float64):
    """[B, 2048] of x [B, 3, H, W] in [0, 1], every operation in `dtype` on x's device."""
    x = x.to(dtype)
    if resize_input:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    if normalize_input:
        x = 2 * x - 1
    return walk(TensorOps(sd, dtype), x)
