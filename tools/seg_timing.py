"""Time source_info's stages on the device: HIP events around
the C-ABI calls with preallocated outputs, 2 warm-ups, median of 7.

Two workloads: one 2048x2048 field with box 64, and 1024 images of 256x256
with box 32 (float32 input, about 1 % of the pixels in Gaussian blobs on
noise, n_pixels 5, threshold 1.5 rms).  The stages are timed one call each:
background (bsgp_background2d), threshold and convolution (sub = data - bkg,
thr = 1.5 rms, bsgp_convolve2d), detection (bsgp_detect_sources: labelling,
then compaction) and measurement (bsgp_segment_catalog); labelling and
compaction are one call, so their split comes from a kernel trace of this
script (profiles/seg/README.md).  Each stage is put beside a device-to-device
copy that moves the bytes the stage must read and write once (inputs read,
outputs written; a copy of n bytes reads n and writes n, so the copy is of half
their sum), and the detection and measurement beside their scipy.ndimage
composition on the host.  The deblend stage (bsgp_deblend_sources on the
detection's labels and the measurement's int_cols) is timed four ways: every
parent, no parent selected (the fixed cost: numbering and relabel), only the
parents that split and only those that do not; only a split parent runs the
single-lane flood, so the last two bound its share.  A last line times the
measurement of an all-true 2048x2048 image, whose one segment is scanned by a
single wave.  The same deblend call is also made through
bsgp_deblend_sources_large with the LDS cap where it is: these workloads hold
no parent over the cap, so the difference is the added launch and the
32 bytes per pixel of stream-ordered workspace.

The crowded 450 x 450 frame (tests/golden/crowded_inputs.npz, source_info with
box 60 and n_pixels 5) has parents over the LDS cap: its deblend stage is timed
with the global-memory path off (bsgp_deblend_sources: those parents are left)
and on (bsgp_deblend_sources_large), with only the parents over the cap, with
the largest of them alone, and beside tests/deblend_ref.py on the host for the
parents over the cap.

    python tools/seg_timing.py --out profiles/seg/timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "beta-sgp_amd"))

import _bsgp as B  # noqa: E402
import segmentation as S  # noqa: E402

torch = B.torch


def field(rng, shape, frac=0.01):
    """Sky 100 with noise of sigma 3 and Gaussian blobs (sigma 1.3, 11 x 11
    stamps of about 30 pixels above the threshold) covering `frac` of the pixels."""
    n, H, W = shape
    d = (100.0 + rng.normal(0.0, 3.0, shape)).astype(np.float32)
    yy, xx = np.mgrid[-5:6, -5:6]
    stamp = np.exp(-(yy * yy + xx * xx) / (2 * 1.3 ** 2)).astype(np.float32)
    k = max(1, int(frac * H * W / 30))
    for i in range(n):
        ys, xs = rng.integers(5, H - 5, k), rng.integers(5, W - 5, k)
        for y, x, a in zip(ys, xs, rng.uniform(20.0, 400.0, k)):
            d[i, y - 5:y + 6, x - 5:x + 6] += np.float32(a) * stamp
    return d


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
    return float(np.median(ms)), [float(m) for m in ms]


def copy_ms(nbytes):
    src = torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src))[0]


def host_composition(sub, thr, kernel, npix):
    """convolve, label, remove small components, relabel and measure with
    scipy.ndimage, image by image; returns the flux sums."""
    from scipy import ndimage
    out = []
    for s, t in zip(sub, thr):
        conv = ndimage.convolve(s, kernel[::-1, ::-1], mode="constant", cval=0.0) / kernel.sum()
        lab, n = ndimage.label(conv > t, structure=np.ones((3, 3), int))
        idx = np.arange(1, n + 1)
        keep = ndimage.sum(np.ones_like(s), lab, idx) >= npix
        new = np.zeros(n + 1, np.int32)
        new[1:][keep] = np.arange(1, keep.sum() + 1)
        lab = new[lab]
        idx = np.arange(1, keep.sum() + 1)
        flux = ndimage.sum(s, lab, idx)
        ndimage.minimum(s, lab, idx), ndimage.maximum(s, lab, idx)
        ndimage.center_of_mass(conv, lab, idx), ndimage.find_objects(lab)
        out.append(float(np.sum(flux)))
    return np.array(out)


def run(name, shape, box, host_images, rng, npix=5, sigma_threshold=1.5):
    n, H, W = shape
    L = B.lib()
    d = torch.from_numpy(field(rng, shape)).cuda()
    ny, nx = H // box, W // box
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    bkg, rms = torch.empty(shape, **f64), torch.empty(shape, **f64)
    mesh, rmesh = torch.empty((n, ny, nx), **f64), torch.empty((n, ny, nx), **f64)
    med = torch.empty((n, 2), **f64)
    st = torch.empty((n, 1 + 3 * ny * nx), **i32)
    sub, thr, conv = torch.empty(shape, **f64), torch.empty(shape, **f64), torch.empty(shape, **f64)
    lab, nlab = torch.empty(shape, **i32), torch.empty((n,), **i32)
    kern = S.make_2dgaussian_kernel(1.2, 3)
    kd = torch.from_numpy(kern).cuda()
    s = B.current_stream

    def background():
        B.check(L.bsgp_background2d(B._ptr(d), B.BSGP_DTYPE_F32, n, H, W, box, box, 3, 3, 3.0, 10,
                                    10.0, 1, None, B._ptr(bkg), B._ptr(rms), B._ptr(mesh),
                                    B._ptr(rmesh), B._ptr(med), B._ptr(st), s()))

    def threshold_conv():
        torch.sub(d, bkg, out=sub)
        torch.mul(rms, sigma_threshold, out=thr)
        B.check(L.bsgp_convolve2d(B._ptr(sub), B.BSGP_DTYPE_F64, n, H, W, B._ptr(kd), 3, 3,
                                  B._ptr(conv), s()))

    def conv_only():
        B.check(L.bsgp_convolve2d(B._ptr(sub), B.BSGP_DTYPE_F64, n, H, W, B._ptr(kd), 3, 3,
                                  B._ptr(conv), s()))

    def detect():
        B.check(L.bsgp_detect_sources(B._ptr(conv), B.BSGP_DTYPE_F64, n, H, W, B._ptr(thr), 0.0, npix,
                                      8, None, B._ptr(lab), B._ptr(nlab), s()))

    t_bkg, _ = timed(background)
    t_thr, _ = timed(threshold_conv)
    t_conv, _ = timed(conv_only)
    t_det, t_det_all = timed(detect)
    counts = nlab.cpu().numpy()
    cap = max(1, int(counts.max()))
    ic, fc = torch.empty((n, cap, 5), **i32), torch.empty((n, cap, 8), **f64)
    cst = torch.empty((n,), **i32)

    def measure():
        B.check(L.bsgp_segment_catalog(B._ptr(sub), B._ptr(conv), B._ptr(lab), n, H, W, cap,
                                       B._ptr(nlab), B._ptr(ic), B._ptr(fc), B._ptr(cst), s()))

    t_cat, _ = timed(measure)
    assert not cst.cpu().numpy().any()

    # deblending: the convolved image, the detection's labels, the measurement's int_cols
    lab2, nlab2, dst = torch.empty(shape, **i32), torch.empty((n,), **i32), torch.empty((n,), **i32)
    sel = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")

    def deblend(select=None):
        B.check(L.bsgp_deblend_sources(B._ptr(conv), B._ptr(lab), n, H, W, cap, B._ptr(nlab),
                                       B._ptr(ic), B._ptr(select), npix, 32, 0.001,
                                       B.BSGP_DEBLEND_EXPONENTIAL, 8, B._ptr(lab2), B._ptr(nlab2),
                                       B._ptr(dst), s()))

    def deblend_large_entry():
        B.check(L.bsgp_deblend_sources_large(B._ptr(conv), B._ptr(lab), n, H, W, cap, B._ptr(nlab),
                                             B._ptr(ic), None, npix, 32, 0.001,
                                             B.BSGP_DEBLEND_EXPONENTIAL, 8, B.BSGP_DEBLEND_MAX_BOX,
                                             B._ptr(lab2), B._ptr(nlab2), B._ptr(dst), s()))

    t_deb, t_deb_all = timed(deblend)
    first = lab2.clone()
    t_deb_le, t_deb_le_all = timed(deblend_large_entry)
    assert torch.equal(first, lab2) and not dst.cpu().numpy().any()
    t_deb, t_deb_all = timed(deblend)  # once more after the other: the pair is taken in one run
    counts2 = nlab2.cpu().numpy()
    over = int((dst.cpu().numpy() & B.BSGP_DEBLEND_OVER_CAP != 0).sum())
    # parent of every output label, hence the parents that split
    par = torch.zeros((n, int(counts2.max()) + 1), **i32)
    par.scatter_(1, lab2.reshape(n, -1).long(), lab.reshape(n, -1))
    kids = torch.zeros((n, cap + 1), **i32)
    live = torch.arange(par.shape[1], device="cuda")[None, :] <= nlab2[:, None]
    kids.scatter_add_(1, par.long(), live.to(torch.int32))
    split = (kids[:, 1:] > 1)
    t_none, _ = timed(lambda: deblend(sel))
    sel_split, sel_rest = split.to(torch.uint8).contiguous(), (~split).to(torch.uint8).contiguous()
    t_split, _ = timed(lambda: deblend(sel_split))
    t_rest, _ = timed(lambda: deblend(sel_rest))
    can_split = int((ic[:, :, 0] >= 2 * npix).sum().item())

    def whole():
        background(), threshold_conv(), detect(), measure()

    t_all, t_all_all = timed(whole)
    px = n * H * W
    areas = ic[:, :, 0].cpu().numpy()
    stage_bytes = {  # inputs read once + outputs written once, per stage
        "background": px * (4 + 16), "threshold_conv": px * (4 + 8 + 8 + 8 + 8 + 8 + 8),
        "convolution_alone": px * 16, "detect": px * (16 + 4), "measure": px * 4 + int(areas.sum()) * 20}
    copies = {k: copy_ms(v / 2) for k, v in stage_bytes.items()}
    # the host composition on the device's own sub / thr maps
    hs, ht = sub[:host_images].cpu().numpy(), thr[:host_images].cpu().numpy()
    t0 = time.perf_counter()
    host_flux = host_composition(hs, ht, kern, npix)
    host_s = time.perf_counter() - t0
    dev_flux = np.array([fc[b, :counts[b], 0].sum().item() for b in range(host_images)])
    r = {
        "workload": name, "images": n, "H": H, "W": W, "box": box, "input": "float32",
        "n_pixels": npix, "segments_kept_total": int(counts.sum()),
        "segments_kept_max_per_image": int(counts.max()),
        "fraction_of_pixels_in_kept_segments": float(areas.sum() / px),
        "ms_background": t_bkg, "ms_threshold_and_convolution": t_thr, "ms_convolution_alone": t_conv,
        "ms_detect_labelling_and_compaction": t_det, "ms_detect_all": t_det_all,
        "ms_measure": t_cat, "ms_all_stages_one_after_another": t_all, "ms_all_stages_all": t_all_all,
        "ms_deblend": t_deb, "ms_deblend_all": t_deb_all,
        "ms_deblend_through_the_large_entry_point": t_deb_le,
        "ms_deblend_through_the_large_entry_point_all": t_deb_le_all,
        "large_entry_point_workspace_bytes": 32 * n * H * W,
        "ms_deblend_no_parent_selected": t_none, "ms_deblend_only_parents_that_split": t_split,
        "ms_deblend_only_parents_that_do_not_split": t_rest,
        "deblend_parents_of_at_least_2_npixels": can_split, "deblend_parents_split": int(split.sum().item()),
        "deblend_labels_out_total": int(counts2.sum()), "deblend_images_with_a_parent_over_the_box_cap": over,
        "stage_bytes_read_plus_written": stage_bytes,
        "ms_d2d_copy_of_half_those_bytes": copies,
        "host_scipy_detect_and_measure_s": host_s, "host_images": host_images,
        "host_s_scaled_to_all_images": host_s * n / host_images,
        "flux_sum_device_vs_host_max_rel": float(np.max(np.abs(dev_flux - host_flux) / np.abs(host_flux))),
    }
    print(json.dumps(r))
    return r


def all_true(H=2048, W=2048):
    """One segment that is the whole field: the union-find's longest paths
    and a single wave scanning 4 Mi pixels twice."""
    L = B.lib()
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    d = torch.ones((1, H, W), **f64)
    lab, nlab = torch.empty((1, H, W), **i32), torch.empty((1,), **i32)
    ic, fc, cst = torch.empty((1, 1, 5), **i32), torch.empty((1, 1, 8), **f64), torch.empty((1,), **i32)
    s = B.current_stream
    t_det, _ = timed(lambda: B.check(L.bsgp_detect_sources(
        B._ptr(d), B.BSGP_DTYPE_F64, 1, H, W, None, 0.5, 1, 8, None, B._ptr(lab), B._ptr(nlab), s())))
    t_cat, _ = timed(lambda: B.check(L.bsgp_segment_catalog(
        B._ptr(d), None, B._ptr(lab), 1, H, W, 1, B._ptr(nlab), B._ptr(ic), B._ptr(fc), B._ptr(cst),
        s())))
    assert int(nlab.cpu()[0]) == 1 and int(ic.cpu()[0, 0, 0]) == H * W
    assert float(fc.cpu()[0, 0, 0]) == float(H * W)
    r = {"workload": f"all-true {H}x{W} (one segment)", "ms_detect": t_det,
         "ms_measure_single_wave": t_cat}
    print(json.dumps(r))
    return r


def crowded(npix=5):
    """The deblend stage of the crowded frame with the global-memory path off and on."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deblend_ref
    with np.load(os.path.join(ROOT, "tests", "golden", "crowded_inputs.npz")) as f:
        img = f["img"].astype(np.float32)
    H, W = img.shape
    L = B.lib()
    cat, _ = S.source_info(img, 60, npix, device_out=True)
    conv = cat.convolved_data.reshape(1, H, W).contiguous()
    lab = cat.segment_img.data.reshape(1, H, W).contiguous()
    ic = cat.int_cols.contiguous()
    cap = ic.shape[1]
    i32 = dict(dtype=torch.int32, device="cuda")
    nlab = torch.tensor([cat.nlabels], **i32)
    lab2, nlab2, dst = torch.empty((1, H, W), **i32), torch.empty((1,), **i32), torch.empty((1,), **i32)
    s = B.current_stream

    def call(large, select=None):
        head = (B._ptr(conv), B._ptr(lab), 1, H, W, cap, B._ptr(nlab), B._ptr(ic), B._ptr(select),
                npix, 32, 0.001, B.BSGP_DEBLEND_EXPONENTIAL, 8)
        tail = (B._ptr(lab2), B._ptr(nlab2), B._ptr(dst), s())
        if large:
            B.check(L.bsgp_deblend_sources_large(*head, B.BSGP_DEBLEND_MAX_BOX, *tail))
        else:
            B.check(L.bsgp_deblend_sources(*head, *tail))

    ich = ic.cpu().numpy()[0]
    box = (ich[:, 2] - ich[:, 1] + 1).astype(np.int64) * (ich[:, 4] - ich[:, 3] + 1)
    over = np.flatnonzero((box > B.BSGP_DEBLEND_MAX_BOX) & (ich[:, 0] >= 2 * npix))
    assert len(over), "no parent over the cap"
    largest = over[np.argmax(ich[over, 0])]

    def select(rows):
        m = np.zeros((1, cap), np.uint8)
        m[0, rows] = 1
        return torch.from_numpy(m).cuda()

    t_off, t_off_all = timed(lambda: call(False))
    n_off, flagged = int(nlab2.cpu()[0]), int(dst.cpu()[0])
    t_on, t_on_all = timed(lambda: call(True))
    n_on = int(nlab2.cpu()[0])
    assert flagged == B.BSGP_DEBLEND_OVER_CAP and int(dst.cpu()[0]) == 0
    sel_over, sel_one, sel_under = select(over), select([largest]), select(np.setdiff1d(np.arange(cap), over))
    t_over, _ = timed(lambda: call(True, sel_over))
    t_one, _ = timed(lambda: call(True, sel_one))
    t_under, _ = timed(lambda: call(True, sel_under))
    call(True, sel_over)
    got = lab2.cpu().numpy()[0]
    ch, lh = conv.cpu().numpy()[0], lab.cpu().numpy()[0]
    t0 = time.perf_counter()
    ref, _, st = deblend_ref.deblend(ch, lh, npix, labels=[int(l) + 1 for l in over])
    host_s = time.perf_counter() - t0
    assert np.array_equal(got, ref)
    r = {"workload": f"crowded frame {H}x{W}, box 60", "n_pixels": npix, "segments": int(cat.nlabels),
         "parents_over_the_lds_cap": len(over),
         "their_boxes": [int(b) for b in box[over]], "their_areas": [int(a) for a in ich[over, 0]],
         "fraction_of_detected_pixels_in_them": float(ich[over, 0].sum() / ich[:, 0].sum()),
         "children_of_them": int(st["nchildren"]), "region_replacements": int(st["splits"]),
         "contrast_removals": int(st["removals"]),
         "labels_out_large_parents_off": n_off, "labels_out_large_parents_on": n_on,
         "ms_deblend_large_parents_off": t_off, "ms_deblend_large_parents_off_all": t_off_all,
         "ms_deblend_large_parents_on": t_on, "ms_deblend_large_parents_on_all": t_on_all,
         "ms_deblend_only_parents_over_the_cap": t_over,
         "ms_deblend_only_parents_under_the_cap_large_entry": t_under,
         "ms_deblend_largest_parent_alone": t_one, "largest_parent_area": int(ich[largest, 0]),
         "largest_parent_box": int(box[largest]),
         "host_restatement_of_parents_over_the_cap_s": host_s}
    print(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B.require_gpu()
    rng = np.random.default_rng(0)
    res = [run("field 2048^2, box 64", (1, 2048, 2048), 64, 1, rng),
           run("1024 x 256^2, box 32", (1024, 256, 256), 32, 32, rng),
           all_true(), crowded()]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
