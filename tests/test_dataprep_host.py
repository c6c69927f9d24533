"""Data preparation, the parts that need no GPU: the numpy oracle (``tests/dataprep_oracle.py``) against ``scipy.ndimage``'s grey morphology,
the thinning table against the rules, the thinning oracle on fixtures written out by hand, the split geometry against a literal loop, and
the error texts of the three entry points."""
import numpy as np
import pytest

from bio_image_unet_amd import dataprep as DP
from tests import dataprep_oracle as DO

FOOTPRINTS = [("disk", 1), ("disk", 2), ("disk", 3), ("disk", 7), ("square", 1), ("square", 2), ("square", 3), ("square", 4)]
SHAPES = [(37, 53), (1, 9), (5, 1)]


def _plane(shape, binary, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) < 0.5) * 255).astype(np.uint8) if binary else rng.integers(0, 256, shape, dtype=np.uint8)


# ---- morphology: the oracle against scipy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,size", FOOTPRINTS)
def test_oracle_morphology_equals_scipy(kernel, size):
    ndi = pytest.importorskip("scipy.ndimage")
    fp = DO.footprint_array(kernel, size)
    for shape in SHAPES:
        for binary in (False, True):
            x = _plane(shape, binary, seed=size + 10 * binary)
            assert np.array_equal(DO.morph(x, "erosion", kernel, size), ndi.grey_erosion(x, footprint=fp, mode="reflect")), (kernel, size, shape, "erosion")
            assert np.array_equal(DO.morph(x, "dilation", kernel, size), ndi.grey_dilation(x, footprint=fp, mode="reflect")), (kernel, size, shape, "dilation")


def test_even_square_example_and_border_rule():
    """The example of the contract: under square(2) a single 255 at (2, 2) dilates to rows and columns 1..2, a single 0 erodes to 2..3; and
    for the disk and the odd square the reflect border equals ignoring positions outside the plane."""
    x = np.zeros((6, 6), dtype=np.uint8)
    x[2, 2] = 255
    d = DO.morph(x, "dilation", "square", 2)
    assert np.array_equal(np.argwhere(d == 255), [[1, 1], [1, 2], [2, 1], [2, 2]])
    e = DO.morph(255 - x, "erosion", "square", 2)
    assert np.array_equal(np.argwhere(e == 0), [[2, 2], [2, 3], [3, 2], [3, 3]])
    x = _plane((9, 11), False, 3)
    for kernel, size in (("disk", 1), ("disk", 2), ("disk", 3), ("square", 3)):
        for op, fill, red in (("erosion", 255, np.minimum), ("dilation", 0, np.maximum)):
            r = 3
            q = np.full((9 + 2 * r, 11 + 2 * r), fill, dtype=np.uint8)
            q[r:-r, r:-r] = x
            acc = np.full(x.shape, fill, dtype=np.uint8)
            for dy, dx in DO.footprint_offsets(kernel, size, op):
                acc = red(acc, q[r + dy:r + dy + 9, r + dx:r + dx + 11])
            assert np.array_equal(DO.morph(x, op, kernel, size), acc), (kernel, size, op)


# ---- thinning ----------------------------------------------------------------------------------------------------------------------------
def test_thin_table_equals_the_rules_entry_by_entry():
    tab = DP.thin_table()
    assert tab.shape == (256,) and tab.dtype == np.uint8
    for n in range(256):
        p = [(n >> k) & 1 for k in range(8)]                  # P2 .. P9 in bits 0 .. 7
        want = int(bool(DO.clears(p, 0))) | (int(bool(DO.clears(p, 1))) << 1)
        assert tab[n] == want, (n, tab[n], want)
    assert tab[0] == 0 and tab[255] == 0                      # isolated and interior pixels stay
    assert tab[0b00000111] & 1 and tab[0b00000111] & 2        # N, NE, E set: a corner, cleared by either sub-iteration


def _grid(rows):
    return np.array([[c == "#" for c in r] for r in rows], dtype=np.uint8)


def test_thinning_oracle_on_hand_written_fixtures():
    """Expected results traced through the rules by hand.  The first sub-iteration takes the south and east boundary and the north-west
    corner, the second the north and west boundary and the south-east corner: the 3 x 7 bar loses its bottom row, both ends of the top row
    and the east end of the middle row, then the rest of the top row and the two new ends of the middle row (the west one has B = 2, the
    east one B = 3, both A = 1) -- four pixels are left, off centre to the west.  The L loses its east column, its bottom row and the two
    outer corners in the first sub-iteration; what is left is one pixel wide, where every pixel has B = 1 or A = 2."""
    bar = _grid([".........",
                 ".#######.",
                 ".#######.",
                 ".#######.",
                 "........."])
    assert np.array_equal(DO.thin(bar), _grid([".........",
                                               ".........",
                                               "..####...",
                                               ".........",
                                               "........."]))
    ell = _grid(["........",
                 ".##.....",
                 ".##.....",
                 ".##.....",
                 ".##.....",
                 ".######.",
                 ".######.",
                 "........"])
    assert np.array_equal(DO.thin(ell), _grid(["........",
                                               "........",
                                               ".#......",
                                               ".#......",
                                               ".#......",
                                               ".#####..",
                                               "........",
                                               "........"]))
    sq2 = _grid(["....", ".##.", ".##.", "...."])
    assert DO.thin(sq2).sum() == 0                            # a 2 x 2 square vanishes
    sq3 = _grid([".....", ".###.", ".###.", ".###.", "....."])
    assert np.array_equal(DO.thin(sq3), _grid([".....", ".....", "..#..", ".....", "....."]))


def test_thinning_oracle_subset_and_idempotent():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    x = ndi.binary_dilation(rng.random((41, 57)) < 0.03, iterations=3).astype(np.uint8)
    t, it = DO.thin(x, return_iterations=True)
    assert it > 1 and 0 < t.sum() < x.sum()
    assert not (t & ~x).any()                                 # a subset of the input
    assert np.array_equal(DO.thin(t), t)                      # a fixed point
    assert DO.thin_step(t, 0)[1] == 0 and DO.thin_step(t, 1)[1] == 0


# ---- split -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("shape", [(20, 300), (64, 64), (32, 64), (70, 130), (200, 50)])
def test_split_2d_equals_a_literal_loop(shape, add):
    dim = (32, 64)
    x = np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)
    # the reference's loop, literally (unet/data.py:192-215)
    merge = np.pad(x, ((0, max(0, dim[0] - shape[0])), (0, max(0, dim[1] - shape[1]))), "reflect")
    dim_in = merge.shape
    N_x, N_y = int(np.ceil(dim_in[0] / dim[0])), int(np.ceil(dim_in[1] / dim[1]))
    N_x += add if N_x > 1 else 0
    N_y += add if N_y > 1 else 0
    X_start = np.linspace(0, dim_in[0] - dim[0], N_x).astype("int16")
    Y_start = np.linspace(0, dim_in[1] - dim[1], N_y).astype("int16")
    want, org = [], []
    for j in range(N_x):
        for k in range(N_y):
            want.append(merge[X_start[j]:X_start[j] + dim[0], Y_start[k]:Y_start[k] + dim[1]])
            org.append((int(X_start[j]), int(Y_start[k])))
    assert DP.origins_2d(shape, dim, add) == org
    assert np.array_equal(DO.split(x, dim, add), np.stack(want))


@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("shape", [(5, 40, 70), (8, 32, 32), (20, 30, 90), (6, 70, 20)])
def test_split_3d_keeps_the_add_patch_quirk(shape, add):
    dim = (8, 32, 32)
    x = np.random.default_rng(2).integers(0, 256, shape, dtype=np.uint8)
    merge = np.pad(x, [(0, max(0, d - s)) for d, s in zip(dim, shape)], "reflect")          # unet3d/data.py:177-200, literally
    dim_in = merge.shape
    N_z, N_x, N_y = (int(np.ceil(dim_in[a] / dim[a])) for a in range(3))
    N_x += add if N_z > 1 else 0
    N_x += add if N_x > 1 else 0
    N_y += add if N_y > 1 else 0
    Z, X, Y = (np.linspace(0, dim_in[a] - dim[a], n).astype("int16") for a, n in enumerate((N_z, N_x, N_y)))
    want, org = [], []
    for j in range(N_z):
        for k in range(N_x):
            for l in range(N_y):
                want.append(merge[Z[j]:Z[j] + dim[0], X[k]:X[k] + dim[1], Y[l]:Y[l] + dim[2]])
                org.append((int(Z[j]), int(X[k]), int(Y[l])))
    assert DP.origins_3d(shape, dim, add) == org
    assert np.array_equal(DO.split(x, dim, add, quirk_3d=True), np.stack(want))
    if add and shape == (20, 30, 90):                         # N_z > 1 makes a one-tile x axis grow, and then grow again
        assert (N_z, N_x, N_y) == (3, 3, 4)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------
def test_error_texts(tmp_path):
    img, msk = np.zeros((8, 8), dtype=np.uint16), np.zeros((8, 8), dtype=np.uint8)
    p = str(tmp_path / "s")
    for fn, a in ((DP.prepare_unet, img), (DP.prepare_unet3d, img[None]), (DP.prepare_siam, np.stack([img, img]))):
        m = msk[None] if fn is DP.prepare_unet3d else msk
        with pytest.raises(ValueError, match="^Number of ground truth does not match number of image stacks$"):
            fn([a, a], [m], p)
        with pytest.raises(ValueError, match="^Dilate kernel star unknown!$"):
            fn([a], [m], p, dilate_kernel="star")
        with pytest.raises(TypeError, match="uint8 or bool"):
            fn([a], [m.astype(np.int16)], p)
    with pytest.raises(NotImplementedError, match="skimage.transform"):
        DP.prepare_siam([np.stack([img, img])], [msk], p, rescale=0.5)
    with pytest.raises(ValueError, match="^Dilate kernel star unknown!$"):
        DO.footprint_offsets("star", 1, "erosion")


def test_signatures_keep_the_reference_keywords():
    import inspect

    import bio_image_unet_amd.siam_unet as siam
    import bio_image_unet_amd.unet as unet
    import bio_image_unet_amd.unet3d as unet3d
    assert unet.prepare is DP.prepare_unet and unet3d.prepare is DP.prepare_unet3d and siam.prepare is DP.prepare_siam
    d = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d(DP.prepare_unet) == dict(dim_out=(256, 256), in_channels=1, out_channels=1, dilate_mask=0, dilate_kernel="disk", add_tile=0, invert=False,
                                      skeletonize=False, clip_threshold=(0.2, 99.8), shiftscalerotate=(0, 0, 0), noise_lims=(0.5, 1.2),
                                      brightness_contrast=(0.25, 0.25), blur_limit=(3, 7), device="auto")
    assert d(DP.prepare_unet3d) == dict(dim_out=(128, 128, 128), dilate_mask=0, dilate_kernel="disk", add_patch=0, invert=False, skeletonize=False,
                                        clip_threshold=(0.2, 99.8), shiftscalerotate=(0, 0, 0), noise_amp=10, brightness_contrast=(0.25, 0.25), device="auto")
    assert d(DP.prepare_siam) == dict(dim_out=(256, 256), dilate_mask=0, dilate_kernel="disk", invert_masks=False, threshold_masks=None, skeletonize=False,
                                      clip_threshold=(0.2, 99.8), shiftscalerotate=(0, 0, 0), noise_amp=10, brightness_contrast=(0.25, 0.25), rescale=None,
                                      device="auto")
