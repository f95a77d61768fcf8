"""Subdivision tiling and mosaic on the device.

The reference's application (application_sgp_subdivisions.py with
restoration/utils.py:332-395) cuts a field into overlapping subdivisions
(``calculate_slice_bboxes`` + astropy ``Cutout2D``), deconvolves each one with
``sgp_betaDiv`` and rebuilds the field with ``reproject_and_coadd``.  Here the
whole chain stays in HBM:

  boxes = calculate_slice_bboxes(...)           # utils.py:332-372, same boxes
  tiles = extract_tiles(field, boxes, shape)    # bsgp_extract_tiles  [n, th, tw]
  out   = sgp.sgp_betaDiv_batch(tiles, ...)     # one batched solve (one workgroup per tile)
  mosaic, footprint = coadd_tiles(out, boxes)   # bsgp_coadd_tiles, mean in tile order

``sgp_subdivisions`` runs the chain.  The co-add is the same-WCS case of
reproject_and_coadd with combine_function='mean'.  ``match_background=True``
adds the reference's ``match_background`` (utils.py:392-397), also on the
device: every tile is solved on its own, so neighbours
disagree by a constant where they overlap and a plain mean leaves a step along
every tile border.  ``tile_pairs`` lists the overlapping pairs (host, integer
geometry), ``match_tile_backgrounds`` takes the median difference of every
pair in its overlap (bit-equal to ``numpy.median``) and solves for the
per-tile corrections: the minimum-norm least-squares solution of
c_i - c_j = O_ij, the fixed point that reproject's shuffled gradient descent
converges to whatever its shuffles, so the step is deterministic here.  The
co-add then takes c_t off tile t.  What stays out: reprojection between grids,
a ``combine_function`` other than the mean, weights, and reproject's NaN
correction for a tile that overlaps no other (it gets 0 and a status bit).
"""
import warnings

import numpy as np

import _bsgp as _B


def calculate_slice_bboxes(image_height, image_width, slice_height=512, slice_width=512,
                           overlap_height_ratio=0.2, overlap_width_ratio=0.2):
    """utils.py:332-372 (same boxes, xyxy, row-major; overlaps int(ratio*size))."""
    boxes = []
    y_max = y_min = 0
    y_overlap = int(overlap_height_ratio * slice_height)
    x_overlap = int(overlap_width_ratio * slice_width)
    while y_max < image_height:
        x_min = x_max = 0
        y_max = y_min + slice_height
        while x_max < image_width:
            x_max = x_min + slice_width
            if y_max > image_height or x_max > image_width:
                xmax = min(image_width, x_max)
                ymax = min(image_height, y_max)
                boxes.append([max(0, xmax - slice_width), max(0, ymax - slice_height), xmax, ymax])
            else:
                boxes.append([x_min, y_min, x_max, y_max])
            x_min = x_max - x_overlap
        y_min = y_max - y_overlap
    return boxes


def subdivision_boxes(shape, subdiv_shape=(100, 100), overlap=10):
    """The boxes create_subdivisions uses (utils.py:378-381: ratio = overlap/size)."""
    return np.asarray(calculate_slice_bboxes(shape[0], shape[1], subdiv_shape[0], subdiv_shape[1],
                                             overlap / subdiv_shape[0], overlap / subdiv_shape[1]),
                      dtype=np.int32)


def tile_centres(boxes):
    """(x, y) pixel centre of every box: ((x0 + x1 - 1) / 2, (y0 + y1 - 1) / 2)."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    return np.stack([(b[:, 0] + b[:, 2] - 1) / 2, (b[:, 1] + b[:, 3] - 1) / 2], axis=1)


def _field(image):
    torch = _B.torch
    if torch.is_tensor(image):
        return image.to(dtype=torch.float64).contiguous()
    return _B.to_dev(np.asarray(image, dtype=np.float64))


def extract_tiles(image, boxes, subdiv_shape):
    """[n, th, tw] float64 CUDA tensor of image[y0:y1, x0:x1] per box."""
    _B.require_gpu()
    torch = _B.torch
    img = _field(image)
    H, W = img.shape
    th, tw = subdiv_shape
    b = np.asarray(boxes, dtype=np.int32).reshape(-1, 4)
    if np.any(b[:, 2] - b[:, 0] != tw) or np.any(b[:, 3] - b[:, 1] != th) or \
            np.any(b[:, :2] < 0) or np.any(b[:, 2] > W) or np.any(b[:, 3] > H):
        raise ValueError("every box must be subdiv_shape sized and inside the field "
                         "(a field smaller than one subdivision yields smaller boxes)")
    bd = torch.from_numpy(np.ascontiguousarray(b)).to("cuda")
    out = torch.empty((len(b), th, tw), dtype=torch.float64, device="cuda")
    _B.check(_B.lib().bsgp_extract_tiles(_B._ptr(img), H, W, _B._ptr(bd), len(b), th, tw,
                                         _B._ptr(out), _B.current_stream()))
    out._keep = (img, bd)
    return out


class TileMatchWarning(UserWarning):
    """The background matching dropped a pair, met a tile without a pair, or
    its solver stopped at the iteration cap."""


class TilePairs:
    """B1, the geometry of the matching (host arrays, int32): ``pairs`` [P, 2]
    (i < j, ordered by (i, j)), ``rects`` [P, 4] their xyxy intersections, the
    adjacency lists ``row_ptr`` [n + 1], ``nbr``, ``nbr_pair``, ``nbr_sign``
    [2 P] (row i: its neighbours in index order, the pair's index, +1 where i
    is the pair's first tile, else -1), ``component`` [n] numbered by their
    first tile, and ``ncomp``."""

    def __init__(self, n, pairs, rects, row_ptr, nbr, nbr_pair, nbr_sign, component, ncomp):
        self.n, self.pairs, self.rects = n, pairs, rects
        self.row_ptr, self.nbr, self.nbr_pair, self.nbr_sign = row_ptr, nbr, nbr_pair, nbr_sign
        self.component, self.ncomp = component, ncomp


def tile_pairs(boxes):
    """Every unordered pair of boxes (xyxy) that intersect in a non-empty
    rectangle -- side and diagonal neighbours, and the inward-shifted edge
    tiles of ``calculate_slice_bboxes`` -- with the adjacency lists and the
    connected components the solver walks (:class:`TilePairs`).  Host only."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    n = len(b)
    pi, pj, rc = [], [], []
    for i in range(n - 1):
        o = b[i + 1:]
        r = np.stack([np.maximum(b[i, 0], o[:, 0]), np.maximum(b[i, 1], o[:, 1]),
                      np.minimum(b[i, 2], o[:, 2]), np.minimum(b[i, 3], o[:, 3])], axis=1)
        hit = np.nonzero((r[:, 2] > r[:, 0]) & (r[:, 3] > r[:, 1]))[0]
        pi.append(np.full(len(hit), i))
        pj.append(hit + i + 1)
        rc.append(r[hit])
    pi = np.concatenate(pi) if pi else np.zeros(0, np.int64)
    pj = np.concatenate(pj) if pj else np.zeros(0, np.int64)
    rects = (np.concatenate(rc) if rc else np.zeros((0, 4))).astype(np.int32).reshape(-1, 4)
    P = len(pi)
    rows, nb = np.concatenate([pi, pj]), np.concatenate([pj, pi])
    order = np.lexsort((nb, rows))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    pair_idx = np.concatenate([np.arange(P), np.arange(P)])[order]
    sign = np.concatenate([np.ones(P), -np.ones(P)])[order]
    parent = list(range(n))  # union-find, the smaller root wins

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    for i, j in zip(pi.tolist(), pj.tolist()):
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    roots = np.asarray([find(k) for k in range(n)], dtype=np.int64)
    _, comp = np.unique(roots, return_inverse=True)  # (roots are first tiles: numbered in order)
    return TilePairs(n, np.stack([pi, pj], axis=1).astype(np.int32).reshape(-1, 2), rects, row_ptr,
                     nb[order].astype(np.int32), pair_idx.astype(np.int32), sign.astype(np.int32),
                     comp.astype(np.int32).reshape(-1), int(comp.max()) + 1 if n else 0)


class TileMatch:
    """The background matching of a set of tiles: ``pairs`` [P, 2] (host),
    ``offsets`` [P] (B2; NaN for a dropped pair), ``corrections`` [n] (B3),
    ``status`` [n] (``_bsgp.BSGP_COADD_*`` bits) and ``solve_info``
    (iterations, relative residual of the conjugate gradients); numpy arrays,
    or CUDA tensors with ``device_out``.  ``geometry`` is the :class:`TilePairs`."""

    def __init__(self, geometry, offsets, corrections, status, solve_info, background_reference):
        self.geometry, self.pairs = geometry, geometry.pairs
        self.offsets, self.corrections, self.status = offsets, corrections, status
        self.solve_info = solve_info
        self.background_reference = background_reference

    def __getitem__(self, key):
        return getattr(self, key)

    @property
    def offset_matrix(self):
        """[n, n] in reproject's layout: O[i, j] = -O[j, i] = the offset of
        pair (i, j), NaN where two tiles do not overlap (and on the diagonal)."""
        n, pr = self.geometry.n, self.pairs
        if _B.torch is not None and _B.torch.is_tensor(self.offsets):
            torch = _B.torch
            m = torch.full((n, n), float("nan"), dtype=torch.float64, device=self.offsets.device)
            if len(pr):
                i = torch.from_numpy(pr[:, 0].astype(np.int64)).to(m.device)
                j = torch.from_numpy(pr[:, 1].astype(np.int64)).to(m.device)
                m[i, j] = self.offsets
                m[j, i] = -self.offsets
            return m
        m = np.full((n, n), np.nan)
        m[pr[:, 0], pr[:, 1]] = self.offsets
        m[pr[:, 1], pr[:, 0]] = -np.asarray(self.offsets)
        return m

    def to_host(self, warn=True):
        """The same match with numpy arrays (waits for the stream); warns on
        the status bits."""
        if _B.torch is not None and _B.torch.is_tensor(self.offsets):
            h = _B.to_host({"o": self.offsets, "c": self.corrections, "s": self.status,
                            "i": self.solve_info})
            m = TileMatch(self.geometry, h["o"], h["c"], h["s"], h["i"], self.background_reference)
        else:
            m = self
        if warn:
            m.warn()
        return m

    def warn(self):
        st = np.asarray(self.status)
        if np.any(st & _B.BSGP_COADD_NONFINITE):
            bad = int(np.sum(~np.isfinite(np.asarray(self.offsets))))
            warnings.warn(f"{bad} pair(s) of tiles with a non-finite value in their overlap were "
                          "left out of the background matching", TileMatchWarning)
        iso = np.nonzero(st & _B.BSGP_COADD_ISOLATED)[0]
        if iso.size:
            warnings.warn(f"{iso.size} tile(s) overlap no other tile (first: {iso[:8].tolist()}): "
                          "their background correction is 0", TileMatchWarning)
        if np.any(st & _B.BSGP_COADD_NOT_CONVERGED):
            warnings.warn("the background corrections did not converge within one iteration per "
                          f"tile (relative residual {float(self.solve_info[1]):.3g})",
                          TileMatchWarning)


def _tiles_boxes(tiles, boxes):
    torch = _B.torch
    t = tiles if torch.is_tensor(tiles) else _B.to_dev(np.asarray(tiles, dtype=np.float64))
    t = t.to(dtype=torch.float64).contiguous()
    b = np.asarray(boxes, dtype=np.int32).reshape(-1, 4)
    if len(b) != t.shape[0]:
        raise ValueError("one box per tile")
    return t, b


_geometry = {}  # (boxes' bytes, device) -> (TilePairs, its device copy, the copy's sections)


def _geometry_dev(b):
    """B1 of boxes ``b`` and its one upload (boxes, pairs, adjacency lists,
    components in one int32 tensor).  The last few layouts are kept: a field's
    image, background and rms mosaics share their boxes (sgp.py:1089-1091), and
    the pair search is host work during which the device would idle."""
    torch = _B.torch
    key = (b.tobytes(), torch.cuda.current_device())
    hit = _geometry.get(key)
    if hit is None:
        g = tile_pairs(b)
        parts = [b.reshape(-1), g.pairs.reshape(-1), g.row_ptr, g.nbr, g.nbr_pair, g.nbr_sign,
                 g.component]
        geo = torch.from_numpy(np.ascontiguousarray(np.concatenate(parts), dtype=np.int32))
        hit = (g, geo.to("cuda"), [len(p) for p in parts])
        if len(_geometry) >= 8:
            _geometry.pop(next(iter(_geometry)))
        _geometry[key] = hit
    return hit


def _match_dev(t, b, background_reference):
    """B1 on the host, B2 and B3 on the device (asynchronous): a TileMatch of
    CUDA tensors, and the device copy of the boxes."""
    torch = _B.torch
    n, th, tw = t.shape
    if np.any(b[:, 2] - b[:, 0] > tw) or np.any(b[:, 3] - b[:, 1] > th) or \
            np.any(b[:, 2] <= b[:, 0]) or np.any(b[:, 3] <= b[:, 1]):
        raise ValueError("every box must be non-empty and no larger than a tile")
    if background_reference is not None:
        k = int(background_reference)
        if k != background_reference or not 0 <= k < n:
            raise ValueError(f"background_reference must be a tile index in 0..{n - 1} or None")
    g, geo, sizes = _geometry_dev(b)
    P = len(g.pairs)
    bd, prd, row_ptr, nbr, nbr_pair, nbr_sign, comp = torch.split(geo, sizes)
    f64 = dict(dtype=torch.float64, device="cuda")
    offsets, corr, info = torch.empty(P, **f64), torch.empty(n, **f64), torch.empty(2, **f64)
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    L, s = _B.lib(), _B.current_stream()
    _B.check(L.bsgp_tile_offsets(_B._ptr(t), n, th, tw, _B._ptr(bd), _B._ptr(prd), P,
                                 _B._ptr(offsets), _B._ptr(status), s))
    _B.check(L.bsgp_tile_corrections(n, _B._ptr(row_ptr), _B._ptr(nbr), _B._ptr(nbr_pair),
                                     _B._ptr(nbr_sign), _B._ptr(comp), g.ncomp, _B._ptr(offsets),
                                     -1 if background_reference is None else int(background_reference),
                                     _B._ptr(corr), _B._ptr(status), _B._ptr(info), s))
    m = TileMatch(g, offsets, corr, status, info, background_reference)
    m._keep = (t, geo)
    return m, bd


def match_tile_backgrounds(tiles, boxes, background_reference=None, device_out=False):
    """The per-tile background corrections of reproject_and_coadd's
    ``match_background=True`` (utils.py:392-397) for tiles [n, th, tw] at
    ``boxes`` on one pixel grid: a :class:`TileMatch`.  ``offsets`` are
    bit-equal to ``numpy.median`` of the two tiles' difference over each
    overlap; ``corrections`` solve c_i - c_j = O_ij in the least-squares sense
    with zero mean in every connected component of the overlap graph, or with
    ``c[background_reference] == 0`` (any tile index: 0 counts, which
    reproject's ``if background_reference:`` overlooks).  Subtract
    ``corrections[t]`` from tile t.  A pair whose overlap holds a non-finite
    difference is dropped, a tile without a pair keeps correction 0; both set
    a status bit and warn (with ``device_out`` nothing waits for the device:
    the bits are in ``status``, and ``to_host()`` warns)."""
    _B.require_gpu()
    t, b = _tiles_boxes(tiles, boxes)
    m, _ = _match_dev(t, b, background_reference)
    return m if device_out else m.to_host()


def coadd_tiles(tiles, boxes, shape, match_background=False, background_reference=None):
    """Mean mosaic [H, W] and footprint [H, W] (tiles covering each pixel).
    ``match_background=True``: the tiles' background corrections
    (:func:`match_tile_backgrounds`, all on the device) are taken off before
    the mean, and ``mean._match`` keeps the :class:`TileMatch` (CUDA tensors)."""
    _B.require_gpu()
    torch = _B.torch
    if match_background:
        t, b = _tiles_boxes(tiles, boxes)
        n, th, tw = t.shape
        m, bd = _match_dev(t, b, background_reference)
        H, W = shape
        mean = torch.empty((H, W), dtype=torch.float64, device="cuda")
        foot = torch.empty((H, W), dtype=torch.float64, device="cuda")
        _B.check(_B.lib().bsgp_coadd_tiles_matched(_B._ptr(t), n, th, tw, _B._ptr(bd),
                                                   _B._ptr(m.corrections), H, W, _B._ptr(mean),
                                                   _B._ptr(foot), _B.current_stream()))
        mean._keep = (t, bd)
        mean._match = m
        return mean, foot
    t = tiles if torch.is_tensor(tiles) else _B.to_dev(np.asarray(tiles, dtype=np.float64))
    t = t.to(dtype=torch.float64).contiguous()
    n, th, tw = t.shape
    b = np.asarray(boxes, dtype=np.int32).reshape(-1, 4)
    if len(b) != n:
        raise ValueError("one box per tile")
    bd = torch.from_numpy(np.ascontiguousarray(b)).to("cuda")
    H, W = shape
    mean = torch.empty((H, W), dtype=torch.float64, device="cuda")
    foot = torch.empty((H, W), dtype=torch.float64, device="cuda")
    _B.check(_B.lib().bsgp_coadd_tiles(_B._ptr(t), n, th, tw, _B._ptr(bd), H, W, _B._ptr(mean),
                                       _B._ptr(foot), _B.current_stream()))
    mean._keep = (t, bd)
    return mean, foot


def _check_bkg_dtype(gn_f32, bkg):
    """A float32 field keeps the reference's float32 arithmetic, where numpy
    also computes the background's share (bkg scaling, sgp.py:648-666) in the
    background's own dtype: tiles cut from a float32 / integer background would
    reach the solve already widened to float64 and silently lose that parity,
    so they raise here as sgp_betaDiv_batch raises for such backgrounds."""
    torch = _B.torch
    if not gn_f32:
        return
    dt = bkg.dtype if torch.is_tensor(bkg) else np.asarray(bkg).dtype
    f64 = dt == torch.float64 if torch.is_tensor(bkg) else (dt.kind == "f" and dt.itemsize == 8)
    if not f64:
        raise ValueError("float32 images in a batch need float64 backgrounds (numpy computes the "
                         "background's part in float32 from a float32 background; solve such "
                         "images one at a time with sgp_betaDiv / sgp)")


def _estimate_bkg(image, bkg, box_size, filter_size):
    """``bkg="estimate"``: the field's background map from background.Background2D
    (utils.py:235-239), estimated once on the device in float64 and left
    there; any other ``bkg`` is returned as it is."""
    if not isinstance(bkg, str):
        return bkg
    if bkg != "estimate":
        raise ValueError(f'bkg must be a scalar, a map or "estimate", got {bkg!r}')
    if box_size is None:
        raise ValueError('bkg="estimate" needs bkg_box_size (Background2D\'s box_size)')
    from background import Background2D
    return Background2D(image, box_size, filter_size=filter_size, device_out=True).background


def _segment_flux(sgp_kwargs, tiles, box_size, repeat=1, localbkg_width=0, deblend=False):
    """``flux="segments"``: every tile's flux constraint becomes the sum of
    ``segment_flux`` of ``source_info(tile, bkg_box_size, n_pixels=5,
    localbkg_width=localbkg_width, deblend=deblend)``
    (application_sgp_subdivisions.py:88,104,113: each subdivision's own
    detection with its own background), all tiles in one batch; any other
    ``flux`` stays as it is."""
    from segmentation import check_localbkg_width
    check_localbkg_width(localbkg_width)
    if not isinstance(sgp_kwargs.get("flux"), str):
        return
    if sgp_kwargs["flux"] != "segments":
        raise ValueError(f'flux must be a number, an array or "segments", got {sgp_kwargs["flux"]!r}')
    if box_size is None:
        raise ValueError('flux="segments" needs bkg_box_size (source_info\'s box_size)')
    from segmentation import segment_flux_sums
    sums = segment_flux_sums(tiles, box_size, n_pixels=5, localbkg_width=localbkg_width,
                             deblend=bool(deblend))
    sgp_kwargs["flux"] = np.repeat(sums, repeat)


def sgp_subdivisions(image, psf, bkg, subdiv_shape=(256, 256), overlap=32, betaParams=None,
                     device_out=False, bkg_box_size=None, bkg_filter_size=(3, 3),
                     flux_localbkg_width=0, flux_deblend=False, match_background=False,
                     background_reference=None, **sgp_kwargs):
    """Field -> overlapping subdivisions -> one batched beta-SGP solve -> mean
    mosaic.  ``bkg``: scalar, or a field-sized map (cut like the image, as the
    application cuts its background map).  ``psf``: one stamp for every tile,
    [n_tiles, kh, kw] stamps, or a DIAPL model (psf_calculate.PSF), which is
    evaluated on the device at every tile centre (field pixel coordinates,
    (x, y) = ((x0 + x1 - 1) / 2, (y0 + y1 - 1) / 2)) so each tile is solved
    with its own PSF.  ``bkg="estimate"`` estimates the map from the field
    itself with background.Background2D(image, bkg_box_size, bkg_filter_size).
    ``flux="segments"`` gives every tile the application's flux constraint, the
    sum of ``segment_flux`` of ``segmentation.source_info(tile, bkg_box_size,
    n_pixels=5, localbkg_width=flux_localbkg_width, deblend=flux_deblend)``;
    ``flux_localbkg_width=5, flux_deblend=True`` is the reference's constraint
    (its catalogue subtracts a local background, utils.py:244-246), the
    defaults 0 and ``False`` leave the sums as they were.
    ``match_background=True`` (with ``background_reference``) co-adds as the
    reference does, the tiles' backgrounds matched first (:func:`coadd_tiles`);
    the solve outputs then carry ``"bkg_match"``, the :class:`TileMatch`.
    Returns (mosaic, footprint, solve outputs); numpy unless device_out."""
    import sgp
    torch = _B.torch
    bkg = _estimate_bkg(image, bkg, bkg_box_size, bkg_filter_size)
    # a float32 field (the application's FITS data) keeps the reference's
    # float32 arithmetic per tile (sgp.py:648-666; include/bsgp.h gn_f32)
    f32 = (image.dtype == torch.float32) if torch.is_tensor(image) else \
        (np.asarray(image).dtype.kind == "f" and np.asarray(image).dtype.itemsize == 4)
    sgp_kwargs.setdefault("gn_f32", bool(f32))
    _check_bkg_dtype(sgp_kwargs["gn_f32"], bkg)
    img = _field(image)
    H, W = img.shape
    boxes = subdivision_boxes((H, W), subdiv_shape, overlap)
    tiles = extract_tiles(img, boxes, subdiv_shape)
    b = np.asarray(bkg) if not torch.is_tensor(bkg) else bkg
    if (torch.is_tensor(b) and b.dim() == 2) or (not torch.is_tensor(b) and b.ndim == 2):
        bk = extract_tiles(b, boxes, subdiv_shape)
    else:
        bk = torch.full((len(boxes),), float(b), dtype=torch.float64, device="cuda")
    if hasattr(psf, "stamps"):  # spatially varying DIAPL model: a stamp per tile centre
        psf = psf.stamps(tile_centres(boxes), normalize=True, device_out=True)
    _segment_flux(sgp_kwargs, tiles, bkg_box_size, localbkg_width=flux_localbkg_width,
                  deblend=flux_deblend)
    out = sgp.sgp_betaDiv_batch(tiles, psf, bk, betaParams=betaParams, device_out=True,
                                **sgp_kwargs)
    mosaic, foot = coadd_tiles(out["x"], boxes, (H, W), match_background=match_background,
                               background_reference=background_reference)
    match = mosaic._match if match_background else None
    if device_out:
        if match_background:
            out["bkg_match"] = match
        return mosaic, foot, out
    torch.cuda.current_stream().synchronize()
    _B.check_status(out["counters"])
    res = {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}
    if match_background:
        res["bkg_match"] = match.to_host()
    return mosaic.cpu().numpy(), foot.cpu().numpy(), res


def sgp_subdivisions_multistart(image, psf, bkg, betas=None, score=None, subdiv_shape=(256, 256),
                                overlap=32, bkg_box_size=None, bkg_filter_size=(3, 3),
                                flux_localbkg_width=0, flux_deblend=False,
                                match_background=False, background_reference=None,
                                **sgp_kwargs):
    """The application's beta search for every subdivision of a field at once
    (application_sgp_subdivisions.py:69-107 per tile): the (tile x candidate)
    product -- n tiles x K initial betas (default: the application's five
    seeds) -- is ONE batched solve, image t*K + k being tile t with beta k;
    each tile keeps the candidate its score ranks best with the application's
    strict running minimum (sgp.argmin_strict), and the mosaic is co-added
    from those.  The application's final re-solve with the best beta repeats
    that candidate's run exactly (the reference is deterministic), so it is
    not run again.

    ``score(x, tile)`` (host arrays of one candidate and its observed tile)
    is the application's photometric score; ``segmentation.flux_fraction_score(
    None, box_size)`` computes it on the device (a score object with a ``batch``
    method gets every candidate in one call); without one the final
    discrepancy ranks the candidates.  ``flux="segments"``,
    ``flux_localbkg_width`` and ``flux_deblend`` as in :func:`sgp_subdivisions`.  ``psf``,
    ``bkg`` (``"estimate"`` with ``bkg_box_size`` included) and the keyword
    arguments as in :func:`sgp_subdivisions`; so are ``match_background`` and
    ``background_reference``, and ``info["bkg_match"]`` then holds the
    :class:`TileMatch` of the chosen candidates.
    Returns (mosaic, footprint, info): info holds the boxes, "betas",
    "scores" [n, K], "best" [n] (candidate index per tile), "best_beta" [n],
    and the solve outputs of the chosen candidates ("x", "iters", "discr",
    "beta_final")."""
    import sgp
    torch = _B.torch
    bkg = _estimate_bkg(image, bkg, bkg_box_size, bkg_filter_size)
    betas = list(sgp.app_beta_candidates() if betas is None else betas)
    K = len(betas)
    f32 = (image.dtype == torch.float32) if torch.is_tensor(image) else \
        (np.asarray(image).dtype.kind == "f" and np.asarray(image).dtype.itemsize == 4)
    sgp_kwargs.setdefault("gn_f32", bool(f32))
    _check_bkg_dtype(sgp_kwargs["gn_f32"], bkg)
    img = _field(image)
    H, W = img.shape
    boxes = subdivision_boxes((H, W), subdiv_shape, overlap)
    n = len(boxes)
    tiles = extract_tiles(img, boxes, subdiv_shape)
    b = np.asarray(bkg) if not torch.is_tensor(bkg) else bkg
    if (torch.is_tensor(b) and b.dim() == 2) or (not torch.is_tensor(b) and b.ndim == 2):
        bk = extract_tiles(b, boxes, subdiv_shape).repeat_interleave(K, dim=0)
    else:
        bk = torch.full((n * K,), float(b), dtype=torch.float64, device="cuda")
    if hasattr(psf, "stamps"):
        psf = psf.stamps(tile_centres(boxes), normalize=True, device_out=True)
    if (psf.dim() if torch.is_tensor(psf) else np.ndim(psf)) == 3:
        pt = psf if torch.is_tensor(psf) else _B.to_dev(np.asarray(psf, dtype=np.float64))
        psf = pt.repeat_interleave(K, dim=0)
    gns = tiles.repeat_interleave(K, dim=0)
    _segment_flux(sgp_kwargs, tiles, bkg_box_size, repeat=K, localbkg_width=flux_localbkg_width,
                  deblend=flux_deblend)
    out = sgp.sgp_betaDiv_batch(gns, psf, bk, betaParams=np.tile(np.asarray(betas, float), n),
                                **sgp_kwargs)
    t_host = tiles.cpu().numpy()
    scores = np.empty((n, K))
    if hasattr(score, "batch"):  # all candidates of all tiles in one batched evaluation
        scores[:] = np.asarray(score.batch(out["x"], gns)).reshape(n, K)
    else:
        for t in range(n):
            for k in range(K):
                i = t * K + k
                it = int(out["iters"][i])
                scores[t, k] = (float(score(out["x"][i], t_host[t])) if score is not None
                                else float(out["discr"][i, it]))
    best = []
    for t in range(n):
        j = sgp.argmin_strict(scores[t])
        if j is None:
            raise ValueError(f"tile {t}: no candidate scores below +inf ({scores[t]})")
        best.append(j)
    best = np.asarray(best)
    pick = np.arange(n) * K + best
    xs = out["x"][pick]
    mosaic, foot = coadd_tiles(xs, boxes, (H, W), match_background=match_background,
                               background_reference=background_reference)
    info = {"boxes": boxes, "betas": betas, "scores": scores, "best": best,
            "best_beta": np.asarray(betas)[best], "x": xs, "iters": out["iters"][pick],
            "discr": out["discr"][pick], "beta_final": out["beta_final"][pick]}
    torch.cuda.current_stream().synchronize()
    if match_background:
        info["bkg_match"] = mosaic._match.to_host()
    return mosaic.cpu().numpy(), foot.cpu().numpy(), info
