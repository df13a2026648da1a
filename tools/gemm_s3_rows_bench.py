"""Stand-alone time of the encoder's output_proj + norms.0 at the production shape (21 950 x 256 x
256): the pair hip.s3_split -> hip.gemm_s3 (row epilogue) against the one launch
hip.gemm_s3_rows_ln that reads the fp32 rows itself, and the two entry splits against the
two-output split.  HIP events over 40 launches, three repetitions in one process (the first is
cold), outputs compared bitwise in the same program.  python tools/gemm_s3_rows_bench.py"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pairnet_amd import hip

DEV = "cuda:0"


def timed(fn, n=40):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main(M=21950, K=256):
    hip.lib()
    torch.manual_seed(0)
    a, w = torch.randn(M, K, device=DEV), torch.randn(256, K, device=DEV) / 16
    bias, res = torch.randn(256, device=DEV), torch.randn(M, 256, device=DEV)
    gamma, beta = torch.rand(256, device=DEV) + 0.5, torch.randn(256, device=DEV)
    pos = torch.randn(M, K, device=DEV)
    n = hip.s3_floats(M, 256)
    ws, rs = torch.empty(hip.s3_floats(256, K), device=DEV), torch.empty(n, device=DEV)
    hip.s3_split(w, ws)
    hip.s3_split(res, rs)
    ss = torch.zeros(hip.s3_floats(M, K), device=DEV)
    ref, got = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    kw = dict(bias=bias, res_s3=rs, gamma=gamma, beta=beta)

    def split():
        hip.s3_split(a, ss)

    def gemm():
        hip.gemm_s3(ss, ws, M, 256, K, out_s3=ref, **kw)

    def pair():
        split()
        gemm()

    def rows():
        hip.gemm_s3_rows_ln(a, ws, M, 256, K, out_s3=got, **kw)

    xs, xps = torch.zeros(hip.s3_floats(M, K), device=DEV), torch.zeros(hip.s3_floats(M, K), device=DEV)
    xs2, xps2 = torch.zeros_like(xs), torch.zeros_like(xps)

    def entry_two():
        hip.s3_split(a, xs)
        hip.s3_split(a, xps, add=pos)

    def entry_one():
        hip.s3_split(a, xs2, add=pos, out_add=xps2)

    for rep in range(3):
        t = [timed(f) for f in (split, gemm, pair, rows, entry_two, entry_one)]
        print("rep %d: s3_split %.1f us, gemm_s3<ln> %.1f us, pair %.1f us | gemm_s3_rows_ln %.1f us | "
              "entry: two splits %.1f us, one launch %.1f us" % ((rep,) + tuple(t)))
    same = torch.equal(ref.view(torch.int32), got.view(torch.int32))
    same_e = torch.equal(xs.view(torch.int32), xs2.view(torch.int32)) and \
        torch.equal(xps.view(torch.int32), xps2.view(torch.int32))
    print("outputs bitwise equal: gemm %s, entry splits %s" % (same, same_e))
    assert same and same_e


if __name__ == "__main__":
    main()
