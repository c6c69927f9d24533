"""Generate ``predict_pins_{unet,unet3d,siam,mo2d}.npz`` in this directory by running the REFERENCE's own ``Predict`` constructors, start to
finish, on the CPU with the position-dependent stub networks of ``tests/predict_pin_stub.py``.

Run in the build container only (the reference is absent on the GPU box), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_predict_pins.py

``unet/predict.py``, ``unet3d/predict.py``, ``siam_unet/predict.py`` and ``multi_output_unet/predict.py`` are loaded by file path.  They import
``tifffile`` (not installed) and, relatively, ``..progress``, ``..utils`` and their model modules, so placeholder modules for those and for the
parent packages are registered in ``sys.modules`` first: the model modules' classes are the stubs, ``..utils.save_as_tif`` keeps the array it
is handed (the 2-D and 3-D results), and for the Siam family ``tifffile`` is a small in-memory fake (``imread(name, key=i)``,
``TiffFile(name).pages[i].shape`` and a ``TiffWriter`` whose ``write`` collects the frames).  The constructors run with ``device='cpu'`` and a
checkpoint written by ``torch.save``, so the fixtures pin their counts, pairing and order too.  ``Predict._Predict__split`` of the loaded class
is wrapped to record what it returns; the reference's code is unchanged.  Only arrays and settings leave this script.

Per geometry ``<name>`` of a family's file (2-D, 3-D and Siam results are uint8, multi-output ones float32 per head):

  <name>.result[.<head>]           the reference's stitched result, in its own dtype
  <name>.N_x / .N_y / .N_z / .X_start / .Y_start / .Z_start        counts and start vectors, as the family has them
  <name>.n_patches, .patches_crc32 number of patches ``__split`` returned (all frames of a Siam movie) and the crc32 of their bytes
  <name>.input_crc32               crc32 of the generated input (the tests regenerate it from the seed)
  <name>.overlapped, .disagreeing  pixels of the result under two or more tiles, and those of them whose tiles predict different values
  3-D:   <name>.plain_mean         the nan-mean over ALL covering patches (no three overwrite layers), uint8; .plain_mean_differs its distance
                                   from the result in voxels
  mo2d:  <name>.fill.<head>, .fill_pixels      the float16 mean of the head's patches and the number of pixels without weight
         <name>.max_weighted_tiles             most tiles with weight on one pixel (the bound's 4)
         <name>.unweighted.a, .cut_origin.a    head a stitched with every weight 1, and (drift only) at the origins the windows were cut at
  meta_json                        the stub module's constants and geometries, ``numpy.__version__`` and the scalar facts above per geometry

Asserted here, on the CPU, so that the fixtures can fail a wrong stitcher: at least a tenth of the overlapped pixels see disagreeing tiles;
the 120-patch 3-D result differs from the plain nan-mean; every multi-tile multi-output result differs from the unweighted mean, and the
drift geometry from a stitch at the cut origins, by more than 1000 x the GPU test's bound (9 x 2^-24 x max|result|); and the float64 mean
and numpy's float16 mean of every head's patches round to the same float16 for the chosen seeds (they do; no seed had to be changed).

Not pinned: a stack of SEVERAL images whose stride yields more windows than ``N_x * N_y``.  Upstream computes ``N_per_img`` from ``N_x * N_y``
while the patch list is longer, so patches of image 0 are stitched into image 1; ``PredictMo2d`` raises ``ValueError`` there.  The
single-image column surplus (``column_surplus``) is recorded as upstream computes it -- its reshape scrambles the tiles -- and
``PredictMo2d`` raises there as well.
"""
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import types
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import predict_pin_stub as S  # noqa: E402

REF = "/root/reference/bio_image_unet"
CAPTURED = {}                 # what save_as_tif was handed
MOVIES, WRITTEN = {}, {}      # the in-memory tifffile of the Siam family


def placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class ProgressNotifier:
    @staticmethod
    def progress_notifier_tqdm():
        return None


class FakeTiffFile:
    def __init__(self, name):
        self.pages = [types.SimpleNamespace(shape=f.shape) for f in MOVIES[name]]


class FakeTiffWriter:
    def __init__(self, name, bigtiff=False):
        self.frames = WRITTEN.setdefault(name, [])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def write(self, arr, contiguous=True):
        self.frames.append(np.array(arr))


def load_reference(package, models):
    """``<package>/predict.py`` of the reference with placeholders for everything it imports but numpy and torch."""
    def save_as_tif(imgs, filename, normalize=False):
        CAPTURED["result"] = np.array(imgs)

    tif = placeholder("tifffile", imread=lambda name, key=None: np.array(MOVIES[name] if key is None else MOVIES[name][key]),
                      TiffFile=FakeTiffFile, TiffWriter=FakeTiffWriter)
    tif.tifffile = placeholder("tifffile.tifffile", TiffFile=FakeTiffFile)
    placeholder("bio_image_unet").__path__ = []
    placeholder(f"bio_image_unet.{package}").__path__ = []
    for mod, classes in models.items():
        placeholder(f"bio_image_unet.{package}.{mod}", **classes)
    placeholder("bio_image_unet.progress", ProgressNotifier=ProgressNotifier)
    placeholder("bio_image_unet.utils", get_device=lambda: torch.device("cpu"), save_as_tif=save_as_tif)
    name = f"bio_image_unet.{package}.predict"
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, package, "predict.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    recorded = []
    split = mod.Predict._Predict__split

    def recording_split(self, arr):
        out = split(self, arr)
        recorded.append(np.array(out))
        return out
    mod.Predict._Predict__split = recording_split
    return mod, recorded


def save_checkpoint(tmp, family, geo):
    path = os.path.join(tmp, "model.pt")
    torch.save(S.checkpoint(family, geo), path)
    return path


def cover_stats(spatial, placements, crop):
    """placements: (origin, tile [C, *extent]) -> (pixels of the cropped canvas under >= 2 tiles, those whose tiles disagree)."""
    cnt = np.zeros(spatial, dtype=np.int64)
    lo, hi = None, None
    for origin, tile in placements:
        tile = np.asarray(tile, dtype=np.float64)
        if lo is None:
            lo, hi = np.full((tile.shape[0],) + tuple(spatial), np.inf), np.full((tile.shape[0],) + tuple(spatial), -np.inf)
        sl = tuple(slice(int(o), int(o) + e) for o, e in zip(origin, tile.shape[1:]))
        cnt[sl] += 1
        lo[(slice(None),) + sl] = np.minimum(lo[(slice(None),) + sl], tile)
        hi[(slice(None),) + sl] = np.maximum(hi[(slice(None),) + sl], tile)
    c = tuple(slice(0, e) for e in crop)
    over = cnt[c] >= 2
    dis = over & (hi[(slice(None),) + c] != lo[(slice(None),) + c]).any(axis=0)
    return int(over.sum()), int(dis.sum())


def u8_outputs(net, patches, batch_view):
    """What the reference's ``__predict`` computes from its uint8 patches: byte / 255, the stub, ``(res * 255).astype('uint8')``."""
    with torch.no_grad():
        return [(net(*(torch.from_numpy(c.astype("float32") / 255).view(batch_view) for c in chans))[0][0].numpy() * 255).astype("uint8")
                for chans in patches]


def check_disagreement(tag, over, dis):
    assert over == 0 or dis * 10 >= over, (tag, over, dis)


def run_unet(tmp):
    R, rec = load_reference("unet", {"unet": {"Unet": S.StubU8}, "unet_v0": {"Unet_v0": S.StubU8}, "attention_unet": {"AttentionUnet": S.StubU8}})
    arrays, facts = {}, {}
    for name, geo in S.GEOMETRIES["unet"].items():
        del rec[:]
        imgs = S.make_input(geo)
        p = R.Predict(imgs.copy(), "unused", save_checkpoint(tmp, "unet", geo), network=S.StubU8, resize_dim=geo["resize_dim"], invert=geo["invert"],
                      normalization_mode=geo["mode"], add_tile=geo["add_tile"], show_progress=False, device="cpu")
        result, (patches,) = CAPTURED.pop("result"), rec
        assert result.dtype == np.uint8 and patches.dtype == np.uint8 and len(patches) == p.N
        th, tw = geo["resize_dim"]
        outs = u8_outputs(S.StubU8(out_channels=geo["out_channels"]), [(q,) for q in patches], (1, 1, th, tw))
        n_img, h, w = geo["shape"]
        over = dis = 0
        for i in range(n_img):
            pl = [((p.X_start[j], p.Y_start[k]), outs[i * p.N_per_img + j * p.N_y + k]) for j in range(p.N_x) for k in range(p.N_y)]
            o, d = cover_stats((max(th, h), max(tw, w)), pl, (h, w))
            over, dis = over + o, dis + d
        check_disagreement(name, over, dis)
        f = dict(N_x=p.N_x, N_y=p.N_y, X_start=p.X_start.tolist(), Y_start=p.Y_start.tolist(), n_patches=len(patches), patches_crc32=S.crc32(patches),
                 input_crc32=S.crc32(imgs), overlapped=over, disagreeing=dis)
        store(arrays, facts, name, f, result=result)
    return arrays, facts


def run_unet3d(tmp):
    R, rec = load_reference("unet3d", {"unet3d": {"UNet3D": S.StubU8}})
    arrays, facts = {}, {}
    for name, geo in S.GEOMETRIES["unet3d"].items():
        del rec[:]
        vol = S.make_input(geo)
        rd = geo["resize_dim"]
        p = R.Predict(vol.copy(), "unused", save_checkpoint(tmp, "unet3d", geo), network=S.StubU8, resize_dim=rd, invert=geo["invert"],
                      add_patch=geo["add_patch"], progress_bar=False, device="cpu")
        result, (patches,) = CAPTURED.pop("result"), rec
        assert result.dtype == np.uint8 and patches.dtype == np.uint8 and len(patches) == p.N
        outs = u8_outputs(S.StubU8(), [(q,) for q in patches], (1, 1) + tuple(rd))
        starts = [(z, x, y) for z in p.Z_start for x in p.X_start for y in p.Y_start]
        canvas = tuple(max(a, b) for a, b in zip(geo["shape"], rd))
        over, dis = cover_stats(canvas, list(zip(starts, outs)), geo["shape"])
        check_disagreement(name, over, dis)
        acc, cnt = np.zeros(canvas), np.zeros(canvas)
        for s, o in zip(starts, outs):
            sl = tuple(slice(int(a), int(a) + e) for a, e in zip(s, rd))
            acc[sl] += o[0]
            cnt[sl] += 1
        plain = (acc / cnt).astype("uint8")[tuple(slice(0, e) for e in geo["shape"])]
        differs = int((plain != result).sum())
        assert differs > 0 or p.N <= 3, (name, differs)           # up to three patches sit in a layer each: the two means are one
        f = dict(N_z=p.N_z, N_x=p.N_x, N_y=p.N_y, Z_start=p.Z_start.tolist(), X_start=p.X_start.tolist(), Y_start=p.Y_start.tolist(),
                 n_patches=len(patches), patches_crc32=S.crc32(patches), input_crc32=S.crc32(vol), overlapped=over, disagreeing=dis,
                 plain_mean_differs=differs, max_cover=int(cnt.max()))
        store(arrays, facts, name, f, result=result, plain_mean=plain)
    return arrays, facts


def run_siam(tmp):
    R, rec = load_reference("siam_unet", {"siam_unet": {"Siam_UNet": S.StubSiam}})
    arrays, facts = {}, {}
    for name, geo in S.GEOMETRIES["siam"].items():
        del rec[:]
        movie = S.make_input(geo)
        MOVIES[name] = movie.copy()
        p = R.Predict(name, name, save_checkpoint(tmp, "siam", geo), resize_dim=geo["resize_dim"], invert=geo["invert"],
                      normalization_mode=geo["mode"], clip_threshold=(0., 99.8), add_tile=geo["add_tile"], show_progress=False, device="cpu")
        result = np.stack(WRITTEN.pop(name))
        patches = np.concatenate(rec)
        T, h, w = geo["shape"]
        th, tw = geo["resize_dim"]
        assert result.dtype == np.uint8 and result.shape == (T, h, w) and patches.shape == (T * p.N, 2, th, tw) and patches.dtype == np.uint8
        outs = u8_outputs(S.StubSiam(), [(q[0], q[1]) for q in patches], (1, 1, th, tw))
        over = dis = 0
        for i in range(T):
            pl = [((p.X_start[j], p.Y_start[k]), outs[i * p.N + j * p.N_y + k]) for j in range(p.N_x) for k in range(p.N_y)]
            o, d = cover_stats((max(th, h), max(tw, w)), pl, (h, w))
            over, dis = over + o, dis + d
        check_disagreement(name, over, dis)
        f = dict(N_x=p.N_x, N_y=p.N_y, X_start=p.X_start.tolist(), Y_start=p.Y_start.tolist(), n_patches=len(patches), patches_crc32=S.crc32(patches),
                 input_crc32=S.crc32(movie), overlapped=over, disagreeing=dis)
        store(arrays, facts, name, f, result=result)
    return arrays, facts


def mo2d_blend(p16, rows, cols, n_y, patch, canvas, weight_of, fill):
    """Head patches [n, C, ph, pw] float16 (the first ``len(rows) * n_y`` are used), tile (j, k) at (rows[j], cols[k]); float64 arithmetic."""
    acc, ws = np.zeros((p16.shape[1],) + canvas), np.zeros(canvas)
    for j, r in enumerate(rows):
        for k, c in enumerate(cols):
            wt = weight_of(j, k)
            sl = (slice(int(r), int(r) + patch[0]), slice(int(c), int(c) + patch[1]))
            acc[(slice(None),) + sl] += p16[j * n_y + k].astype(np.float64) * wt
            ws[sl] += wt
    out = np.where(ws > 0, acc / np.where(ws > 0, ws, 1), fill)
    return out, ws


def run_mo2d(tmp):
    R, rec = load_reference("multi_output_unet", {"multi_output_nested_unet": {"MultiOutputNestedUNet": S.StubHeads2D,
                                                                              "MultiOutputNestedUNet_3Levels": S.StubHeads2D}})
    arrays, facts = {}, {}
    for name, geo in S.GEOMETRIES["mo2d"].items():
        del rec[:]
        imgs = S.make_input(geo)
        p = R.Predict(imgs.copy(), save_checkpoint(tmp, "mo2d", geo), result_path=None, network=S.StubHeads2D, max_patch_size=geo["max_patch_size"],
                      batch_size=S.MO2D_BATCH, add_tile=geo["add_tile"], show_progress=False, device="cpu")
        (patches,) = rec
        n_img, h, w = geo["shape"]
        ph, pw = p.patch_size
        assert patches.dtype == np.float32 and patches.shape[1:] == (ph, pw) and (n_img == 1 or len(patches) == p.N)
        with torch.no_grad():
            out = S.StubHeads2D(output_heads=S.HEADS)(torch.from_numpy(np.ascontiguousarray(patches))[:, None])
        p16 = {k: v.numpy().astype("float16") for k, v in out.items()}
        canvas = (max(ph, h), max(pw, w))
        m = 20

        def weight_of(j, k):
            wt = np.ones((ph, pw))
            if j > 0:
                wt[:m] = 0
            if j < p.N_x - 1:
                wt[-m:] = 0
            if k > 0:
                wt[:, :m] = 0
            if k < p.N_y - 1:
                wt[:, -m:] = 0
            return wt
        f = dict(patch_size=[ph, pw], N_x=p.N_x, N_y=p.N_y, X_start=p.X_start.tolist(), Y_start=p.Y_start.tolist(), n_patches=len(patches),
                 patches_crc32=S.crc32(patches), input_crc32=S.crc32(imgs), fill={}, bound={}, unweighted_differs={})
        extra = {}
        over = dis = 0
        for i in range(n_img):
            pl = [((p.X_start[j], p.Y_start[k]), p16["b"][i * p.N_per_img + j * p.N_y + k]) for j in range(p.N_x) for k in range(p.N_y)]
            o, d = cover_stats(canvas, pl, (h, w))
            over, dis = over + o, dis + d
        check_disagreement(name, over, dis)
        f.update(overlapped=over, disagreeing=dis)
        for k, head in S.HEADS.items():
            res = p.result[k]
            assert res.dtype == np.float32 and res.min() >= 0 and res.max() < 1
            mean16 = p16[k].mean()
            assert mean16.dtype == np.float16 and np.float16(p16[k].astype(np.float64).mean()) == mean16, (name, k, "change the seed")
            f["fill"][k] = float(mean16)
            f["bound"][k] = bound = 9 * 2.0 ** -24 * float(np.abs(res).max())
            res4 = res.reshape(n_img, head["channels"], h, w)
            crop = (slice(None), slice(0, h), slice(0, w))
            for i in range(n_img):
                own, ws = mo2d_blend(p16[k][i * p.N_per_img:], p.X_start, p.Y_start, p.N_y, (ph, pw), canvas, weight_of, float(mean16))
                assert np.abs(own[crop] - res4[i]).max() <= bound, (name, k)          # this script's restatement reads the fixture right
                assert np.array_equal(res4[i][:, ws[crop[1:]] == 0], np.full_like(res4[i][:, ws[crop[1:]] == 0], np.float32(mean16)))
                if i == 0:
                    f["fill_pixels"] = int((ws[crop[1:]] == 0).sum())
                    cover = np.zeros(canvas)
                    for j, r in enumerate(p.X_start):
                        for c_, c in enumerate(p.Y_start):
                            cover[int(r):int(r) + ph, int(c):int(c) + pw] += weight_of(j, c_)
                    f["max_weighted_tiles"] = int(cover.max())
                    assert f["max_weighted_tiles"] <= 4
            if p.N_per_img > 1 and k == "a":
                plain = np.stack([mo2d_blend(p16[k][i * p.N_per_img:], p.X_start, p.Y_start, p.N_y, (ph, pw), canvas, lambda j, c: np.ones((ph, pw)), 0.)[0][crop]
                                  for i in range(n_img)]).astype("float32")
                f["unweighted_differs"][k] = d = float(np.abs(plain.astype(np.float64) - res4).max())
                assert d > 1000 * bound, (name, k, d, bound)
                extra["unweighted.a"] = np.squeeze(plain)
                if name == "drift":
                    sx = int(p.X_start[1])
                    cut_rows = [j * sx for j in range(p.N_x)]
                    assert cut_rows == [0, 26, 52] and p.X_start.tolist() == [0, 26, 53]
                    alt = mo2d_blend(p16[k], cut_rows, p.Y_start, p.N_y, (ph, pw), canvas, weight_of, float(mean16))[0][crop].astype("float32")
                    f["cut_origin_differs"] = d = float(np.abs(alt.astype(np.float64) - res4[0]).max())
                    assert d > 1000 * bound, (name, d, bound)
                    extra["cut_origin.a"] = np.squeeze(alt)
        store(arrays, facts, name, f, **{f"result.{k}": p.result[k] for k in S.HEADS}, **extra)
    return arrays, facts


def store(arrays, facts, name, f, **named):
    facts[name] = f
    for k, v in named.items():
        arrays[f"{name}.{k}"] = np.asarray(v)
    for k, v in f.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                arrays[f"{name}.{k}.{kk}"] = np.asarray(vv)
        else:
            arrays[f"{name}.{k}"] = np.asarray(v, dtype=np.float64 if isinstance(v, float) else np.int64)
    print(name, json.dumps(f))


def save_npz(path, arrays):
    """An ``.npz`` with fixed member order and time stamps, so that a rerun reproduces the file byte for byte (``np.savez`` stamps the clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asarray(arrays[key]), allow_pickle=False)


def main():
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(tmp)                                   # the Siam constructor makes a temp_<name> folder where it stands
    try:
        for family, run in (("unet", run_unet), ("unet3d", run_unet3d), ("siam", run_siam), ("mo2d", run_mo2d)):
            print(f"== {family}")
            arrays, facts = run(tmp)
            meta = dict(S.meta(), family=family, numpy=np.__version__, facts=facts)
            arrays["meta_json"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
            out = os.path.join(HERE, f"predict_pins_{family}.npz")
            save_npz(out, arrays)
            print(out, os.path.getsize(out), "bytes")
            assert os.path.getsize(out) < (1 << 20)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
