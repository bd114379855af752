"""Time the three-filter scattering layers (the entry points of csrc/scat.hip with their third filter) and what the third filter path costs.

    python tools/scat_rot_bench.py [--out profiles/scat_rot_bench.txt]

Taps from the test fixtures (tests/golden/golden_rot_dtcwt.npz: near_sym_b_bp 13, 19, 19 taps + qshift_b_bp 14 taps; no tap
provider is needed), 'symmetric', magbias 1e-2, the shapes of profiles/scat_bench.txt: (8,1,256,256), (64,1,256,256), (8,1,512,512);
``ScatLayer`` and ``ScatLayerj2`` forward + backward (a cotangent on Z).  Three tables:
  (a) the three-filter layer against the plain-torch restatement of tests/test_rot_cpu.py run on the device in fp32;
  (b) the three-filter layer against the two-filter layer on the same bank's first two filters (same tap counts, same tiles): what
      the third path costs;
  (c) the two-filter layers on near_sym_a + qshift_a, the bank and the method of tools/scat_bench.py, beside the fused medians
      that profiles/scat_bench.txt records (its "(a) composed" rows) -- the two-filter kernels compile to the same instructions as
      before the third path existed, so the two columns differ by the run-to-run spread only.
A row: median [min, max] ms of either side, the ratio of the medians and the spread (max - min) / median of the seven batches of
either.  Method (tools/dwt_bench.py's): 5 warm-up runs of each, then 7 batches of 20 runs each, the two sides' batches
alternating, timed with device events around the batch; outputs are not read back between runs.
"""
import argparse
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import faoctasr                          # noqa: E402
from dwt_bench import timed_pair         # noqa: E402
import test_rot_cpu as R                 # noqa: E402
import test_scat_cpu as S                # noqa: E402

SHAPES = ((8, 1, 256, 256), (64, 1, 256, 256), (8, 1, 512, 512))


def recorded(path):
    """{(shape, layer): fused median ms} of the "(a) composed" rows of profiles/scat_bench.txt."""
    out = {}
    if os.path.exists(path):
        for line in open(path):
            m = re.match(r"(\S+)\s+(ScatLayer\w*)\s+fused ([0-9.]+) \[([0-9.]+), ([0-9.]+)\]\s+\(a\)", line)
            if m:
                out[m.group(1), m.group(2)] = tuple(float(m.group(k)) for k in (3, 4, 5))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scat_rot_bench.txt"))
    args = ap.parse_args()
    faoctasr._lib.load()
    b64 = R.bufs()
    fb, fq = R.tuples(b64)
    b = {k: v.float().cuda() for k, v in b64.items()}
    one3, two3 = faoctasr.ScatLayer(biort=fb).cuda(), faoctasr.ScatLayerj2(biort=fb, qshift=fq).cuda()
    one2, two2 = faoctasr.ScatLayer(biort=fb[:2]).cuda(), faoctasr.ScatLayerj2(biort=fb[:2], qshift=fq[:4]).cuda()
    ab, aq = S.tuples("a")
    onea, twoa = faoctasr.ScatLayer(biort=ab).cuda(), faoctasr.ScatLayerj2(biort=ab, qshift=aq).cuda()
    old = recorded(os.path.join(ROOT, "profiles", "scat_bench.txt"))
    lines = ["Three-filter scattering layers, near_sym_b_bp (13, 19, 19 taps) + qshift_b_bp (14 taps), 'symmetric', forward + backward, device: %s;"
             % torch.cuda.get_device_name(0), "median [min, max] ms of 7 batches of 20 runs; spread = (max - min) / median of the batches, left / right", ""]

    def row(shape, what, lname, left, rname, right, tail=""):
        (m, lo, hi), (tm, tlo, thi) = timed_pair(left, right)
        lines.append("%-16s %-12s %-12s %.4f [%.4f, %.4f]  %-12s %.4f [%.4f, %.4f]  ratio %6.2fx  spread %4.1f%% / %4.1f%%%s"
                     % ("x".join(map(str, shape)), what, lname, m, lo, hi, rname, tm, tlo, thi, tm / m, 100 * (hi - lo) / m, 100 * (thi - tlo) / tm, tail))
        print(lines[-1], flush=True)
        return m, lo, hi

    def steps(xg, mods):
        cot = torch.randn_like(mods[0](xg))

        def step(fn):
            def run():
                xg.grad = None
                fn(xg).backward(cot)
            return run
        return [step(m) for m in mods]

    for title, table in (("(a) three-filter fused against the plain-torch restatement on the device", "a"),
                         ("(b) three-filter against two-filter, same bank less its third filters (ratio < 1: the third path's cost)", "b"),
                         ("(c) two-filter near_sym_a + qshift_a against itself, beside the medians profiles/scat_bench.txt records", "c")):
        lines += [title]
        print(title, flush=True)
        for shape in SHAPES:
            xg = torch.randn(*shape, device="cuda").requires_grad_(True)
            for what, m3, m2, ma, plain in (("ScatLayer", one3, one2, onea, lambda t: R.layer1(t, b, "symmetric")),
                                            ("ScatLayerj2", two3, two2, twoa, lambda t: R.layer2(t, b))):
                if table == "a":
                    f, p = steps(xg, [m3, plain])
                    row(shape, what, "3-filter", f, "torch", p)
                elif table == "b":
                    f, g = steps(xg, [m3, m2])
                    row(shape, what, "3-filter", f, "2-filter", g)
                else:
                    f, g = steps(xg, [ma, ma])
                    rec = old.get(("x".join(map(str, shape)), what))
                    row(shape, what, "2-filter", f, "again", g, "  recorded %.4f [%.4f, %.4f]" % rec if rec else "  recorded: none")
        lines.append("")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
