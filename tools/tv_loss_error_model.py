"""Where the error bar of tests/test_gpu_tv_loss.py comes from: the summation order of csrc/tv.hip emulated in fp32 numpy on the
CPU, against the fp32 reference's own distance from float64, over every shape the GPU test uses.

The emulation follows the kernels thread for thread: the (plane, strip of 8 rows, column group) work items, each thread's running
sums over its rows (a fused multiply-add per term: the product is exact in double, one rounding to fp32), the 64-lane xor
butterfly, the four waves added left to right, and the final kernel's double sums.  The backward is a stencil with no sum; its
fp32 arithmetic is restated term for term.  e_ref is the fixture's error for the fixture shapes (the reference's own CPU
result) and the fp32 torch composition's on the CPU for the others.

    python tools/tv_loss_error_model.py            # prints the table recorded in profiles/tv_loss_error.txt
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_tv.npz")
ROWS = 8
SWEEP = ((8, 1, 256, 256), (2, 1, 192, 192), (3, 1, 63, 50), (2, 2, 96, 64), (1, 1, 2, 2), (1, 1, 2, 257), (1, 1, 130, 2))
f32 = np.float32


def composition(x, weight, dtype):
    """The reference's formula with stock ops on the CPU in ``dtype``: (loss, gradient) as float64."""
    x = x.detach().to(dtype).requires_grad_(True)
    b, c, h, w = x.shape
    h_tv = torch.pow(x[:, :, 1:, :] - x[:, :, :h - 1, :], 2).sum()
    w_tv = torch.pow(x[:, :, :, 1:] - x[:, :, :, :w - 1], 2).sum()
    loss = weight * 2 * (h_tv / (c * (h - 1) * w) + w_tv / (c * h * (w - 1))) / b
    g, = torch.autograd.grad(loss, x)
    return float(loss.detach().double()), g.double()


def fma(acc, d):
    """acc + d * d with one rounding (d * d is exact in double; the double sum's own rounding is 2^-29 of an fp32 ulp)."""
    return (acc.astype(np.float64) + d.astype(np.float64) * d.astype(np.float64)).astype(f32)


def emulate_forward(x, weight):
    x = x.numpy().astype(f32)
    B, C, H, W = x.shape
    V = 4 if W % 4 == 0 else 1
    planes = x.reshape(B * C, H, W)
    strips, WV = (H + ROWS - 1) // ROWS, W // V
    items = B * C * strips * WV
    blocks = (items + 255) // 256
    q = np.arange(items)
    c0, t = (q % WV) * V, q // WV
    r0, p = (t % strips) * ROWS, t // strips
    sh, sw = np.zeros(items, f32), np.zeros(items, f32)
    for r in range(ROWS + 1):
        ok = r0 + r < H
        row = np.minimum(r0 + r, H - 1)
        if r < ROWS:
            for k in range(V):
                has = ok & (c0 + k + 1 < W)
                d = planes[p, row, np.minimum(c0 + k + 1, W - 1)] - planes[p, row, c0 + k]
                sw = np.where(has, fma(sw, d), sw)
        if r > 0:
            for k in range(V):
                d = planes[p, row, c0 + k] - planes[p, row - 1, c0 + k]
                sh = np.where(ok, fma(sh, d), sh)

    def block_sums(v):
        v = np.concatenate([v, np.zeros(blocks * 256 - items, f32)]).reshape(blocks * 4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ o]
        w4 = v[:, 0].reshape(blocks, 4)
        return ((w4[:, 0] + w4[:, 1]) + w4[:, 2]) + w4[:, 3]
    a, b = block_sums(sh).astype(np.float64).sum(), block_sums(sw).astype(np.float64).sum()
    return float(f32(2.0 * weight * (a / (C * (H - 1) * W) + b / (C * H * (W - 1))) / B))


def emulate_backward(x, weight):
    x = x.numpy().astype(f32)
    B, C, H, W = x.shape
    s = 2.0 * weight / B
    kh, kw = f32(s * 2.0 / (C * (H - 1) * W)), f32(s * 2.0 / (C * H * (W - 1)))
    a, b = np.zeros_like(x), np.zeros_like(x)
    a[:, :, 1:, :] += x[:, :, 1:, :] - x[:, :, :-1, :]
    a[:, :, :-1, :] -= x[:, :, 1:, :] - x[:, :, :-1, :]
    b[:, :, :, 1:] += x[:, :, :, 1:] - x[:, :, :, :-1]
    b[:, :, :, :-1] -= x[:, :, :, 1:] - x[:, :, :, :-1]
    return torch.from_numpy((kh * a + kw * b).astype(np.float64))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def rows():
    g = np.load(GOLD)
    for shape in g["shapes"]:
        tag = "%dx%dx%dx%d" % tuple(shape)
        x = torch.from_numpy(g["x_" + tag])
        for w in g["weights"]:
            yield "fixture %s w%g" % (tag, w), x, float(w), float(g["loss_w%g_%s" % (w, tag)]), torch.from_numpy(g["g_w%g_%s" % (w, tag)])
    for shape in SWEEP:
        B, C, H, W = shape
        x = torch.tanh(torch.randn(*shape, generator=torch.Generator().manual_seed(77 + H + 3 * C + W)))
        l32, g32 = composition(x, 1.0, torch.float32)
        yield "B%d C%d %dx%d" % shape, x, 1.0, l32, g32


def main():
    worst_l = worst_g = 0.0
    for name, x, w, l32, g32 in rows():
        l64, g64 = composition(x, w, torch.float64)
        ulp = abs(l64) * 2.0 ** -23
        e_ref, e_emu = abs(l32 - l64), abs(emulate_forward(x, w) - l64)
        eg_ref, eg_emu = rel_l2(g32, g64), rel_l2(emulate_backward(x, w), g64)
        worst_l, worst_g = max(worst_l, e_emu / e_ref), max(worst_g, eg_emu / eg_ref)
        print("%-28s loss %.7f e_ref %.3e (%.2f ulp) e_emu %.3e (%.2f ulp) ratio %.2f | grad e_ref %.3e e_emu %.3e ratio %.3f"
              % (name, l64, e_ref, e_ref / ulp, e_emu, e_emu / ulp, e_emu / e_ref, eg_ref, eg_emu, eg_emu / eg_ref))
    print("worst ratio e_emu / e_ref: loss %.3f, gradient %.3f  ->  K = twice that: loss %.2f, gradient %.2f" % (worst_l, worst_g, 2 * worst_l, 2 * worst_g))


if __name__ == "__main__":
    sys.exit(main())
