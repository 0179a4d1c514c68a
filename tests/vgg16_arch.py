"""The published layer list of VGG16's convolutional part (Simonyan and Zisserman 2015, configuration D; torchvision's
`vgg16().features`), restated for the tests: torchvision is not installed.  Every convolution is 3 x 3, stride 1, padding 1, with a bias
and a ReLU behind it; "M" is a 2 x 2 max pool of stride 2 (floor)."""

CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def layers(upto=30):
    """[(index in `features`, kind, cin, cout)], kind in ("conv", "relu", "pool"), for features[0:upto]."""
    out, cin = [], 3
    for v in CFG:
        if v == "M":
            out.append((len(out), "pool", cin, cin))
        else:
            out.append((len(out), "conv", cin, v))
            out.append((len(out), "relu", v, v))
            cin = v
    return out[:upto]


# LPIPS taps: the outputs of ReLU 1_2, 2_2, 3_3, 4_3, 5_3
LPIPS_TAPS = (3, 8, 15, 22, 29)
LPIPS_WIDTHS = (64, 128, 256, 512, 512)
CONV_INDICES = tuple(i for i, kind, _a, _b in layers() if kind == "conv")      # 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28


def random_state(seed, dtype=None):
    """A seeded state dict under torchvision's names plus lin{0..4} [1, C, 1, 1]: He-normal filters, small biases, lin in [0, 0.1]."""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for i, kind, cin, cout in layers():
        if kind == "conv":
            sd["features.%d.weight" % i] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
            sd["features.%d.bias" % i] = torch.randn(cout, generator=g) * 0.1
    for k, c in enumerate(LPIPS_WIDTHS):
        sd["lin%d" % k] = torch.rand(1, c, 1, 1, generator=g) * 0.1
    return sd if dtype is None else {k: v.to(dtype) for k, v in sd.items()}
