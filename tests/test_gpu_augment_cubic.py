"""Cubic-spline resampling of rotated targets on the GPU: ``biu_spline_prefilter_f32`` and ``biu_augment_f32_cubic`` through the C ABI against
the float64 oracle (``tests/augment_cubic_oracle.py``, pinned to scipy by ``tests/test_augment_cubic_host.py``), then the augmenter, the feeder
and ``TrainerMo2d`` that carry them.  Every test prints its figures before it asserts.

Shapes ``[planes, H, W]``: (1, 8, 12) both extents below the prefilter's reach R = 16, the halo wraps repeatedly; (3, 19, 37) odd, unaligned
rows, the element-wise store path and a range over several planes; (2, 64, 64) exactly one tile, the vector store path; (1, 70, 130) partial
tiles on both axes.

Bounds (none of them comes from what the kernels give):

* coefficients and the cubic gather: the rule of ``tests/test_gpu_augment_f32.py``.  The kernel's largest deviation from the float64 oracle
  (the exact periodic prefilter) is at most ``MARGIN = 6`` times the largest deviation of the fp32 numpy restatement (sum cut at R, fp32 taps,
  weights and sums, the kernel's order of additions) from the same oracle on the same inputs; the margin covers fused multiply-adds and
  another operation order, not a wrong tap.  Every pixel is compared: the interpolant is continuous in the coordinate.
* value range, samples without an arbitrary angle, the augmenter and the feeder: bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bio_image_unet_amd import augment as A  # noqa: E402
from bio_image_unet_amd._lib import check, lib  # noqa: E402
from bio_image_unet_amd.feed import DeviceFeeder, TileStore  # noqa: E402
from tests import augment_cubic_oracle as CO  # noqa: E402
from tests import augment_f32_oracle as FO  # noqa: E402

SHAPES = [(1, 8, 12), (3, 19, 37), (2, 64, 64), (1, 70, 130)]                                    # [planes, H, W]
SOURCES = ["f32", "u8"]
FIELDS = ["unit", "mask", "wide"]              # values in [0.02, 0.98] (clip active), 0 / 1 (clip essential), [-3, 5] (no clip; f32 only)
# angle in degrees, scale, shift in pixels: angle alone, angle with scale != 1 and a whole-pixel shift
ROTATING = [(17.3, 1, 0, 0), (151, 1.0731, 5, -3), (203.7, 0.9137, -4, 6), (359, 1.1913, 12, 12)]
MARGIN = 6.0
ids = lambda s: s if isinstance(s, str) else "x".join(map(str, s))
CASES = [(shape, source, field) for shape in SHAPES for source in SOURCES for field in FIELDS if not (source == "u8" and field == "wide")]
case_ids = ["-".join((ids(s), src, f)) for s, src, f in CASES]


def _field(shape, source, field, seed):
    rng = np.random.default_rng(seed)
    if field == "mask":
        on = rng.random(shape) > 0.5
        return on.astype(np.float32) if source == "f32" else (on * 255).astype(np.uint8)
    if field == "wide":
        return (-3.0 + 8.0 * rng.random(shape)).astype(np.float32)
    if source == "u8":
        return rng.integers(5, 251, size=shape, dtype=np.uint8)
    return (0.02 + 0.96 * rng.random(shape)).astype(np.float32)


def _geo(index, h, w, g):
    angle, scale, dx, dy = g
    return A.record_f32(index, h, w, angle=angle if angle else None, scale=scale if scale != 1 else None, shift=(dx, dy))


def _plain(h, w):
    """Records without an arbitrary angle: a quarter turn, scale only, shift only, nothing."""
    return [A.record_f32(20, h, w, rot_k=1 if h == w else 2), A.record_f32(21, h, w, scale=1.0731), A.record_f32(22, h, w, shift=(3, -2)),
            A.record_f32(23, h, w)]


@functools.lru_cache(maxsize=None)
def case(shape, source, field):
    """A batch of 6: the four rotating geometries with a quarter turn and a scale-only sample between them, and its references, computed
    once: the float64 oracle and the fp32 restatement of coefficients and output."""
    p, h, w = shape
    plain = _plain(h, w)
    recs = np.stack([_geo(0, h, w, ROTATING[0]), plain[0], _geo(2, h, w, ROTATING[1]), _geo(3, h, w, ROTATING[2]), plain[1], _geo(5, h, w, ROTATING[3])])
    batch = np.stack([_field(shape, source, field, 50 + i) for i in range(len(recs))])
    rot = np.array([bool(int(r["flags"]) & A.ROT_F) for r in recs])
    loaded = np.stack([FO.widen(f) for f in batch])
    ref = {"rot": rot, "loaded": loaded,
           "coef64": CO.prefilter_periodic(loaded[rot]), "coef32": CO.prefilter_truncated(loaded[rot], CO.R, np.float32),
           "out64": np.stack([CO.apply_mask_cubic(f, r)[0] for f, r in zip(batch, recs)]),
           "out32": np.stack([CO.apply_mask_cubic(f, r, np.float32)[0] for f, r in zip(batch, recs)])}
    for v in ref.values():
        v.setflags(write=False)
    return batch, recs, ref


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _params(recs):
    return torch.from_numpy(np.ascontiguousarray(recs, dtype=A.PARAMS_F32_DTYPE).view(np.uint8).copy()).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run_cubic(batch, recs):
    """``batch`` [N, P, H, W] float32 or uint8 -> (coef, range, output) of the two-call path as numpy arrays; unwritten elements stay 7."""
    n, p, h, w = batch.shape
    src, par = _dev(batch), _params(recs)
    coef = torch.full(batch.shape, 7.0, dtype=torch.float32, device="cuda")
    rng = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda")
    dst = torch.full(batch.shape, 7.0, dtype=torch.float32, device="cuda")
    u8 = int(batch.dtype == np.uint8)
    check(lib.biu_spline_prefilter_f32(C.c_void_p(src.data_ptr()), u8, C.c_void_p(coef.data_ptr()), C.c_void_p(rng.data_ptr()), n, p, h, w,
                                       C.c_void_p(par.data_ptr()), _stream()), "spline_prefilter_f32")
    check(lib.biu_augment_f32_cubic(C.c_void_p(src.data_ptr()), u8, C.c_void_p(coef.data_ptr()), C.c_void_p(rng.data_ptr()),
                                    C.c_void_p(dst.data_ptr()), n, p, h, w, C.c_void_p(par.data_ptr()), _stream()), "augment_f32_cubic")
    torch.cuda.synchronize()
    return coef.cpu().numpy(), rng.cpu().numpy(), dst.cpu().numpy()


def _run_linear(batch, recs):
    """``biu_augment_f32(kind = MASK)``."""
    n, p, h, w = batch.shape
    src, par = _dev(batch), _params(recs)
    dst = torch.full(batch.shape, 7.0, dtype=torch.float32, device="cuda")
    check(lib.biu_augment_f32(C.c_void_p(src.data_ptr()), int(batch.dtype == np.uint8), C.c_void_p(dst.data_ptr()), n, p, h, w, FO.MASK,
                              C.c_void_p(par.data_ptr()), 0, 0, 0, 1, _stream()), "augment_f32")
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


@pytest.mark.parametrize("shape,source,field", CASES, ids=case_ids)
def test_coefficients_range_and_cubic_gather(shape, source, field):
    """Coefficients and the gathered, clipped output within six times the fp32 restatement's deviation from the float64 oracle; the value
    range exact; samples without an arbitrary angle bit-equal to ``biu_augment_f32``'s MASK output; a second run gives the same bits."""
    batch, recs, ref = case(shape, source, field)
    rot = ref["rot"]
    coef, rng, out = _run_cubic(batch, recs)
    c_rest = float(np.abs(ref["coef32"].astype(np.float64) - ref["coef64"]).max())
    c_err = float(np.abs(coef[rot].astype(np.float64) - ref["coef64"]).max())
    o_rest = float(np.abs(ref["out32"].astype(np.float64) - ref["out64"])[rot].max())
    o_err = float(np.abs(out.astype(np.float64) - ref["out64"])[rot].max())
    want_rng = np.stack([ref["loaded"][rot].min(axis=(1, 2, 3)), ref["loaded"][rot].max(axis=(1, 2, 3))], axis=1)
    print(f"cubic {shape} {source} {field}: coefficients kernel max |diff| {c_err:.3e}, fp32 restatement {c_rest:.3e}, bound {MARGIN * c_rest:.3e}; "
          f"output kernel {o_err:.3e}, restatement {o_rest:.3e}, bound {MARGIN * o_rest:.3e}; range {rng[rot].tolist()}")
    assert _same(rng[rot], want_rng)
    assert c_rest > 0 and c_err <= MARGIN * c_rest
    assert o_rest > 0 and o_err <= MARGIN * o_rest
    if field != "wide":                                                            # the clip: nothing leaves the sample's own range
        assert all(out[i].min() >= want_rng[j, 0] and out[i].max() <= want_rng[j, 1] for j, i in enumerate(np.flatnonzero(rot)))
    linear = _run_linear(batch, recs)
    assert _same(out[~rot], linear[~rot])
    assert not _same(out[rot], linear[rot])
    again = _run_cubic(batch, recs)
    assert _same(again[0][rot], coef[rot]) and _same(again[1][rot], rng[rot]) and _same(again[2], out)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_samples_without_an_arbitrary_angle(shape, source):
    """Quarter turns, scale only, shift only, or nothing, in one batch with rotating samples: bit-equal to ``biu_augment_f32(kind=MASK)``."""
    p, h, w = shape
    plain = _plain(h, w)
    recs = np.stack([plain[0], _geo(1, h, w, ROTATING[1]), plain[1], plain[2], _geo(4, h, w, ROTATING[0]), plain[3], A.record_f32(6, h, w, rot_k=2, shift=(w + 3, -h - 2))])
    batch = np.stack([_field(shape, source, "unit", 80 + i) for i in range(len(recs))])
    rot = np.array([bool(int(r["flags"]) & A.ROT_F) for r in recs])
    _, _, out = _run_cubic(batch, recs)
    linear = _run_linear(batch, recs)
    diff = int((out[~rot] != linear[~rot]).sum())
    print(f"plain {shape} {source}: {int((~rot).sum())} samples without an arbitrary angle, elements differing from biu_augment_f32 {diff}")
    assert diff == 0 and _same(out[~rot], linear[~rot])
    assert _same(out[5], FO.widen(batch[5]))                                          # nothing drawn: the sample passes unchanged
    assert _same(out[6], np.roll(FO.widen(batch[6])[:, ::-1, ::-1], (-h - 2, w + 3), axis=(1, 2)))       # a half turn, then a shift that wraps


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_zero_angle_with_the_flag_set_returns_the_source(shape, source):
    p, h, w = shape
    rows = []
    for field in FIELDS[:2] + (["wide"] if source == "f32" else []):
        recs = np.stack([A.record_f32(i, h, w, angle=0.0) for i in range(4)])
        assert all(int(r["flags"]) & A.ROT_F for r in recs)
        batch = np.stack([_field(shape, source, field, 90 + i) for i in range(4)])
        loaded = np.stack([FO.widen(f) for f in batch]).astype(np.float64)
        rest = float(np.abs(np.stack([CO.apply_mask_cubic(f, r, np.float32)[0] for f, r in zip(batch, recs)]).astype(np.float64) - loaded).max())
        err = float(np.abs(_run_cubic(batch, recs)[2].astype(np.float64) - loaded).max())
        print(f"identity {shape} {source} {field}: kernel max |diff| from the source {err:.3e}, fp32 restatement {rest:.3e}, bound {MARGIN * rest:.3e}")
        rows.append((field, err, rest))
    for field, err, rest in rows:
        assert rest > 0 and err <= MARGIN * rest, (field, err, rest)


# ---- augmenter ---------------------------------------------------------------------------------------------------------------------------
def _dict_batch(n, hw, seed):
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0, 2 * np.pi, (n,) + hw)
    return {"image": _dev(rng.integers(0, 256, (n,) + hw, dtype=np.uint8)),
            "mask": _dev((rng.random((n, 1) + hw) > 0.5).astype(np.float32)),
            "distance": _dev((rng.random((n,) + hw) * 30 - 2).astype(np.float32)),
            "orientation": _dev(np.stack([np.cos(phi), np.sin(phi)], axis=1).astype(np.float32))}


def test_augmenter_with_cubic_targets():
    hw, n = (32, 48), 6
    batch = _dict_batch(n, hw, 0)
    lin, cub = A.AugmenterF32(shape=hw, seed=9, scale_limit=(-0.1, 0.2)), A.AugmenterF32(shape=hw, seed=9, scale_limit=(-0.1, 0.2), target_interp="cubic")
    recs = cub.draw(1, np.arange(n))
    rot = (recs["flags"] & A.ROT_F) != 0
    print(f"augmenter: {int(rot.sum())} of {n} samples under an arbitrary angle")
    assert rot.any() and not rot.all()
    a, b = lin(batch, recs, 1), cub(batch, recs, 1)
    torch.cuda.synchronize()
    for k in ("image", "orientation"):
        assert torch.equal(a[k], b[k]), k
    for k in ("mask", "distance"):
        src = batch[k].cpu().numpy().reshape(n, 1, *hw)
        direct = _run_cubic(src, recs)[2].reshape(b[k].shape)
        assert _same(b[k].cpu().numpy(), direct), k
        assert _same(a[k].cpu().numpy()[~rot], b[k].cpu().numpy()[~rot]) and not torch.equal(a[k], b[k]), k
    m = b["mask"].cpu().numpy()
    assert m.min() == 0.0 and m.max() == 1.0 and ((m > 0) & (m < 1)).any()                    # clipped, and smooth in between
    again = cub(batch, recs, 1)
    torch.cuda.synchronize()
    assert all(torch.equal(again[k], b[k]) for k in b)
    assert len(cub._spline_scratch) == 2                                                       # one scratch per field, reused
    # no rotating record in the batch: the linear launches, the linear bits
    still = np.stack([A.record_f32(i, *hw, rot_k=2 * (i % 2), scale=1.05 if i % 3 else None, shift=(i, -i), gauss_sigma=0.05) for i in range(n)])
    a, b = lin(batch, still, 2), cub(batch, still, 2)
    torch.cuda.synchronize()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert len(cub._spline_scratch) == 2


# ---- feeder and TrainerMo2d --------------------------------------------------------------------------------------------------------------
HEADS = {"mask": {"channels": 1, "activation": "sigmoid", "loss": "BCEDiceLoss", "weight": 1.0},
         "distance": {"channels": 1, "activation": "relu", "loss": "WeightedDistanceGradientLoss", "weight": 0.25}}


def _store(tmp_path, n=8, hw=(32, 32)):
    """8 tiles of 32 x 32: the image as bytes and two float32 targets."""
    st = TileStore.create(str(tmp_path / "t"), n, {"image": hw, "mask": (1,) + hw, "distance": hw},
                          {"dim_out": list(hw), "scale_limit": [-0.1, 0.1], "random_rotate": True}, dtypes={"mask": "f32", "distance": "f32"})
    rng = np.random.default_rng(0)
    st.maps["image"][:] = rng.integers(0, 256, (n,) + hw)
    st.maps["mask"][:] = rng.random((n, 1) + hw) > 0.5
    st.maps["distance"][:] = rng.random((n,) + hw) * (rng.random((n,) + hw) < 0.6)
    st.flush()
    return st


def test_feeder_with_cubic_targets(tmp_path):
    st = _store(tmp_path)
    mk = lambda: A.AugmenterF32.from_store(st, seed=5, target_interp="cubic")
    idx = [3, 1, 4, 7, 5, 0, 2, 6]
    got = [{k: v.cpu().clone() for k, v in b.items()} for b in DeviceFeeder(st, idx, 4, "cuda", augmenter=mk())]
    aug, lin, rotated, differ = mk(), A.AugmenterF32.from_store(st, seed=5), 0, 0
    assert len(got) == 2
    for b, g in enumerate(got):
        ids_b = idx[4 * b:4 * b + 4]
        recs = aug.draw(0, ids_b)
        raw = {k: v.cuda() for k, v in st.batch_u8(ids_b).items()}
        want, other = aug(raw, recs, 0), lin(raw, recs, 0)
        assert all(torch.equal(want[k].cpu(), g[k]) for k in g)
        rotated += int(((recs["flags"] & A.ROT_F) != 0).sum())
        differ += int(not torch.equal(other["distance"].cpu(), g["distance"]))
    print(f"feeder: {rotated} of {len(idx)} samples under an arbitrary angle, {differ} of {len(got)} batches differ from the linear augmenter's")
    assert rotated > 0 and differ > 0


@pytest.mark.timeout(300)
def test_trainer_mo2d_records_the_target_interpolation(tmp_path):
    from bio_image_unet_amd.workflow import TrainerMo2d
    st = _store(tmp_path)
    kw = dict(batch_size=2, output_heads=HEADS, n_filter=8, device="cuda", val_split=0.25)      # 6 tiles train, 2 validate: one batch
    own = A.AugmenterF32.from_store(st, seed=5, target_interp="cubic")
    torch.manual_seed(3)
    tr = TrainerMo2d(st, 1, save_dir=str(tmp_path / "c"), augment=own, **kw)
    assert tr.augmenter is own and tr.train_loader.augmenter is own
    tr.start()
    ck = torch.load(str(tmp_path / "c" / "model.pt"), weights_only=False)
    print(f"TrainerMo2d(augment=AugmenterF32(target_interp='cubic')): best validation loss after one epoch {float(ck['best_loss']):.6f}")
    assert torch.isfinite(torch.as_tensor(ck["best_loss"]))
    assert ck["online_augmentation"]["target_interp"] == "cubic" and ck["online_augmentation"] == own.describe()
    torch.manual_seed(3)
    tr = TrainerMo2d(st, 1, save_dir=str(tmp_path / "l"), augment=True, **kw)
    assert tr.augmenter.target_interp == "linear"
    tr.start()
    assert torch.load(str(tmp_path / "l" / "model.pt"), weights_only=False)["online_augmentation"]["target_interp"] == "linear"


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def test_arguments_are_validated():
    """Null, overlapping and unaligned pointers, non-positive extents and 2^31 elements return a status and launch nothing: what the launches
    would write keeps its poison."""
    n, p, h, w = 2, 2, 32, 32
    src = torch.rand(n, p, h, w, dtype=torch.float32, device="cuda")
    coef, dst = torch.full_like(src, 7.0), torch.full_like(src, 7.0)
    rng = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda")
    par = _params(np.stack([A.record_f32(i, h, w, angle=17.3) for i in range(n)]))
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off) if t is not None else None

    def pre(s=src, c=coef, r=rng, q=par, dims=(n, p, h, w), s_off=0, c_off=0, r_off=0, u8=0):
        return lib.biu_spline_prefilter_f32(P(s, s_off), u8, P(c, c_off), P(r, r_off), *dims, P(q), _stream())

    def gat(s=src, c=coef, r=rng, d=dst, q=par, dims=(n, p, h, w), s_off=0, c_off=0, r_off=0, d_off=0):
        return lib.biu_augment_f32_cubic(P(s, s_off), 0, P(c, c_off), P(r, r_off), P(d, d_off), *dims, P(q), _stream())

    bad_dims = [(0, p, h, w), (n, 0, h, w), (n, p, -1, w), (n, p, h, 0), (1 << 15, 1, 256, 256), (n, p, 1 << 15, 1 << 14)]
    refused = [pre(s=None), pre(c=None), pre(r=None), pre(q=None), pre(c=src), pre(r=src), pre(r=coef), pre(s=coef, s_off=64),
               pre(s_off=2), pre(c_off=2), pre(r_off=1)] + [pre(dims=d) for d in bad_dims]
    refused += [gat(s=None), gat(c=None), gat(r=None), gat(d=None), gat(q=None), gat(d=src), gat(d=coef), gat(d=rng), gat(d=coef, d_off=16),
                gat(s_off=2), gat(c_off=2), gat(r_off=3), gat(d_off=2)] + [gat(dims=d) for d in bad_dims]
    torch.cuda.synchronize()
    print(f"arguments: {len(refused)} bad calls, statuses {sorted(set(refused))}; last message {lib.biu_last_error()!r}")
    assert all(s != 0 for s in refused)
    assert bool((coef == 7).all()) and bool((rng == 7).all()) and bool((dst == 7).all())
    assert pre(u8=1, s_off=1, dims=(1, 1, h, w)) == 0                                  # bytes need no alignment
    assert pre() == 0 and gat() == 0
    torch.cuda.synchronize()
    assert not bool((coef == 7).any()) and not bool((rng == 7).any()) and not bool((dst == 7).any())
    aug = A.AugmenterF32(shape=(h, w), target_interp="cubic")
    with pytest.raises(ValueError):
        aug({"mask": src}, aug.draw(0, [0, 1]), 0, out={"mask": src})
