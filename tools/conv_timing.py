"""Time bsgp_convolve2d_ex on the device: HIP events around the
C-ABI call with preallocated outputs, 2 warm-ups, median of 7.

Shapes: 30 x 375^2 under 31 x 31 (degrade on the application's tiles),
1024 x 256^2 under 25 x 25, one 2048^2 under 31 x 31, 64 x 31^2 under 31 x 31
(scale_psf) and 1024 x 256^2 under 3 x 3.  Each is timed on finite input (the
plain rule) and with one NaN per image (the interpolating rule), and put beside

* Plan.apply (BSGP_CONV_LINEAR_FILL) on the same shape and kernel: the FFT
  operator, which is not bit-defined and has no NaN rule;
* bsgp_convolve2d for the 3 x 3;
* the arithmetic count 2 * kh * kw * H * W * B separately rounded float64
  operations, as a fraction of the rate a register-only multiply-add loop
  reaches in the same process (tools/conv_rate_probe.hip).

    python tools/conv_timing.py --build-probe        # no device needed
    python tools/conv_timing.py --out profiles/convolve/timing.json
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "beta-sgp_amd"))
PROBE_SRC = os.path.join(ROOT, "tools", "conv_rate_probe.hip")
PROBE_LIB = os.path.join(ROOT, "tools", "_conv_rate_probe.so")

SHAPES = [("degrade_tiles", (30, 375, 375), (31, 31)), ("batch_256", (1024, 256, 256), (25, 25)),
          ("field_2048", (1, 2048, 2048), (31, 31)), ("scale_psf", (64, 31, 31), (31, 31)),
          ("batch_256_3x3", (1024, 256, 256), (3, 3))]


def build_probe():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                    "-ffp-contract=off", PROBE_SRC, "-o", PROBE_LIB], check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--build-probe", action="store_true", help="compile the rate probe and exit")
    args = ap.parse_args()
    if args.build_probe:
        build_probe()
        return
    import _bsgp as B
    torch = B.torch
    B.require_gpu()
    if not os.path.exists(PROBE_LIB):
        build_probe()
    L = B.lib()
    P = ctypes.CDLL(PROBE_LIB)
    vp = ctypes.c_void_p
    P.conv_rate_probe.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp]
    s = B.current_stream

    def timed(fn, warm=2, reps=7):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), [round(float(m), 4) for m in ms]

    # the register-only rate: 256 CUs x 8 workgroups of 256 threads, 16 operations per iteration
    blocks, iters = 256 * 8, 20000
    pout = torch.empty(blocks * 256, dtype=torch.float64, device="cuda")
    pk = torch.full((8,), 1e-9, dtype=torch.float64, device="cuda")
    t_probe, all_probe = timed(lambda: P.conv_rate_probe(B._ptr(pout), B._ptr(pk), blocks, iters, s()))
    rate = 16.0 * iters * blocks * 256 / (t_probe * 1e-3)
    res = {"probe": {"ms": t_probe, "all_ms": all_probe, "ops_per_s": rate}, "shapes": {}}
    print(f"register-only multiply-add loop: {rate / 1e12:.2f} T separately rounded f64 op/s")

    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, (n, H, W), (kh, kw) in SHAPES:
        d = torch.randn((n, H, W), dtype=torch.float64, device="cuda", generator=gen) * 3.0 + 10.0
        dn = d.clone()
        dn[:, H // 2, W // 2] = float("nan")
        k = rng.uniform(0.1, 1.0, (kh, kw))
        kd = torch.from_numpy(k).cuda()
        sd = torch.from_numpy(np.array([k.sum()])).cuda()
        out = torch.empty_like(d)
        st = torch.empty((n,), dtype=torch.int32, device="cuda")

        def direct(x):
            B.check(L.bsgp_convolve2d_ex(B._ptr(x), B.BSGP_DTYPE_F64, n, H, W, B._ptr(kd), kh, kw, 0,
                                         B._ptr(sd), None, B.BSGP_CONV_F_NORMALIZE, 0.0, B._ptr(out),
                                         B._ptr(st), s()))

        t_plain, all_plain = timed(lambda: direct(d))
        assert int(st.max()) == 0
        t_nan, all_nan = timed(lambda: direct(dn))
        assert int(st.min()) == B.BSGP_CONV_HAD_NAN
        ops = 2.0 * kh * kw * H * W * n
        row = {"B": n, "H": H, "W": W, "kh": kh, "kw": kw, "direct_ms": t_plain,
               "direct_all_ms": all_plain, "direct_nan_ms": t_nan, "direct_nan_all_ms": all_nan,
               "ops": ops, "fraction_of_probe_rate": ops / (t_plain * 1e-3) / rate}
        if kh <= 7:
            t_old, _ = timed(lambda: B.check(L.bsgp_convolve2d(B._ptr(d), B.BSGP_DTYPE_F64, n, H, W,
                                                               B._ptr(kd), kh, kw, B._ptr(out), s())))
            row["convolve2d_ms"] = t_old
        try:
            plan = B.Plan(H, W, k / k.sum(), B.BSGP_CONV_LINEAR_FILL)
            t_fft, _ = timed(lambda: plan.apply(d))
            row["plan_apply_ms"] = t_fft
            del plan
        except Exception as e:  # a shape the FFT operator does not take
            row["plan_apply_error"] = str(e)
        res["shapes"][name] = row
        print(name, json.dumps({k_: (round(v, 4) if isinstance(v, float) else v)
                                for k_, v in row.items() if not k_.endswith("all_ms")}))
        del d, dn, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
