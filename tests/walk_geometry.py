"""Shapes at which the persistent convolution kernels WALK: every block of a launch takes a first, a middle and a last brick, and some
blocks stop one round before their neighbours.

A persistent launch has g = min(grid rule(CUs, columns), bricks) blocks per column; block b runs bricks b, b + g, b + 2g, ...  This module
mirrors the grid rules and brick sizes of the launch functions (one table, ROWS: each row names the function it mirrors) and searches the
smallest extents with

    rounds * g < bricks,   bricks % g != 0,   bricks % g <= g / 2            (rounds = 3; 2 for the first layer)

whose extents are not multiples of the brick.  Pure Python: the CU count comes from the caller
(torch.cuda.get_device_properties(0).multi_processor_count on the GPU, fixed numbers in tests/test_walk_geometry_host.py)."""
import math
from collections import namedtuple

GMAC_BUDGET = 15.0          # forward multiply-accumulates of the fp64 CPU reference of one case (conv3d fp64: ~7 GMAC in 0.15 s on 16 threads)


def grid_per_column(budget, cols):
    """biu_conv_mfma.hip: grid_per_column -- a multiple of 8 (XCD-grouped walk) unless rounding down idles more than 1/32 of the chip."""
    exact = budget // cols
    r8 = exact & ~7
    g = exact if (exact - r8) * cols * 32 > budget else r8
    return max(g, 8)


def pick_nt(ntiles):
    """biu_conv_mfma.hip: pick_nt -- output tiles per block."""
    return 2 if ntiles % 2 == 0 else 1


def _g_pairs(cus, pairs):
    g = cus // pairs
    if g >= 16:
        g = grid_per_column(cus, pairs)
    return max(g, 1)


def _g_c1m(cus, cols):
    return 3 * cus


def _g_roll(cus, cols):
    g = max(cus // cols, 1)
    if g & 7 and g > 8:
        g &= ~7
    return g


# brick = (TD, TH, TW) voxels of the tensor the launch walks; TD = None: an item is a whole (H, W) window column over the depth (batch)
# wide: True = the form is taken when W % 32 == 0, False = when it is not, None = W is free
Row = namedtuple("Row", "mirrors brick rule wide")
ROWS = {
    # k_conv_pipe, 3x3x3 and 3x3 (forward; data gradient = the same launch with the channel counts swapped): columns = ntiles / NT
    "conv3d_nt1_wide": Row("launch_conv -> launch_cfg_r<KD=3, 4, 8, 32, NT=1>", (4, 8, 32), grid_per_column, True),
    "conv3d_nt1_narrow": Row("launch_conv -> launch_cfg_r<KD=3, 4, 16, 16, NT=1>", (4, 16, 16), grid_per_column, False),
    "conv3d_nt2": Row("launch_conv -> launch_cfg_r<KD=3, 4, 8, 16, NT=2>", (4, 8, 16), grid_per_column, None),
    "conv2d_nt1_wide": Row("launch_conv / launch_conv_xs -> launch_cfg_r<KD=1, 1, 32, 32, NT=1>", (1, 32, 32), grid_per_column, True),
    "conv2d_nt1_narrow": Row("launch_conv / launch_conv_xs -> launch_cfg_r<KD=1, 1, 64, 16, NT=1>", (1, 64, 16), grid_per_column, False),
    "conv2d_nt2_wide": Row("launch_conv / launch_conv_xs -> launch_cfg_r<KD=1, 1, 16, 32, NT=2>", (1, 16, 32), grid_per_column, True),
    "conv2d_nt2_narrow": Row("launch_conv / launch_conv_xs -> launch_cfg_r<KD=1, 1, 32, 16, NT=2>", (1, 32, 16), grid_per_column, False),
    # fp32 3x3x3 as split bf16 products (biu_set_fp32_products_3d): one output tile per block, columns = ntiles
    "conv3d_x3": Row("launch_conv_x3_3d -> launch_cfg_r<f32x3_t, 4, 8, 16, NT=1>", (4, 8, 16), grid_per_column, None),
    "conv3d_x6": Row("launch_conv_x3_3d -> launch_cfg_r<f32x6_t, 4, 4, 16, NT=1>", (4, 4, 16), grid_per_column, None),
    # k_conv16_pipe (bf16): columns = Cout / (16 * MTL)
    "conv16_3d": Row("launch_conv16<3, 4, 8, MTL> (m16_grid_x)", (4, 8, 16), grid_per_column, None),
    "conv16_2d": Row("launch_conv16<1, 1, 32, MTL> (m16_grid_x)", (1, 32, 16), grid_per_column, None),
    # ConvTranspose k2 s2 on k_conv_pipe, bricks on the COARSE tensor: forward columns = (ntiles / NT) * parities, data gradient ntiles / NT
    "convt3d_fwd": Row("launch_convt_fwd -> launch_cfg_r<1, 1, 1, 4, 8, 16>, nz = 8", (4, 8, 16), grid_per_column, None),
    "convt2d_fwd": Row("launch_convt_fwd -> launch_cfg_r<1, 1, 1, 1, 32, 16>, nz = 4", (1, 32, 16), grid_per_column, None),
    "convt3d_dgrad": Row("launch_convt_dgrad -> launch_cfg_r<2, 2, 2, 2, 8, 16> (biu_mfma_convt_dgrad_rows)", (2, 8, 16), grid_per_column, None),
    "convt2d_dgrad": Row("launch_convt_dgrad -> launch_cfg_r<1, 2, 2, 1, 16, 16> (biu_mfma_convt_dgrad_rows)", (1, 16, 16), grid_per_column, None),
    # nearest x2 folded into the 3x3x3 convolution, bricks on the COARSE tensor: forward columns = (ntiles / NT) * 8, data gradient ntiles / NT
    "upconv_fwd": Row("launch_upconv_cfg -> launch_cfg_r<2, 2, 1, 4, 8, 16>, nz = 8 (biu_mfma_upconv_stat_rows)", (4, 8, 16), grid_per_column, None),
    "upconv_dgrad": Row("launch_upconv_cfg -> launch_cfg_r<2, 2, 1, 4, 8, 16>, nz = 1 (biu_mfma_upconv_dgrad_rows)", (4, 8, 16), grid_per_column, None),
    # weight gradient of the folded up-sampling: k_wgrad_pipe per parity class on the COARSE grid, columns = (dy tiles / NI) x (x tiles)
    "upconv_wgrad_f32": Row("biu_mfma_upconv_wgrad -> launch_wgrad<float, 2, 2, 1, 4, 4, 16, 1, NI> (NI = 2: dy wider than 32 channels)", (4, 4, 16), _g_pairs, None),
    "upconv_wgrad_bf16": Row("biu_mfma_upconv_wgrad -> launch_wgrad<bf16_t, 2, 2, 1, 4, 8, 16, 1, NI> (fused form; NI as above)", (4, 8, 16), _g_pairs, None),
    # k_wgrad_pipe: columns = (dy tiles) x (x tiles) pairs of one launch
    "wgrad3d_f32": Row("launch_wgrad<float, 3, 3, 1, 4, 4, 16, 1>", (4, 4, 16), _g_pairs, None),
    "wgrad3d_bf16": Row("launch_wgrad<bf16_t, 3, 3, 1, 4, 8, 16, 1> (depth < 8: below wroll_fits)", (4, 8, 16), _g_pairs, None),
    "wgrad3d_rr16": Row("launch_wgrad<bf16_t, 3, 3, 1, 4, 8, 16, 1, 1, RR16> (Cin = 16, paired taps)", (4, 8, 16), _g_pairs, None),
    "wgrad2d_f32": Row("launch_wgrad<float | f32x3_t | f32x6_t, 1, 3, 1, 1, 16, 16, 4>", (1, 16, 16), _g_pairs, None),
    "wgrad2d_bf16": Row("launch_wgrad<bf16_t, 1, 3, 1, 1, 16, 32, 4> (batch < 8: below wroll2d_fits)", (1, 16, 32), _g_pairs, None),
    # k_wgrad_roll: an item is an 8 x 16 window over the whole depth (2-D: over the whole batch)
    "wgrad_roll3d": Row("launch_wgrad_roll (depth >= 8, >= 8 windows)", (None, 8, 16), _g_pairs, None),
    "wgrad_roll2d": Row("launch_wgrad_roll(k2d) (batch >= 8 is the depth axis)", (None, 8, 16), _g_pairs, None),
    # k_conv_roll: an item is an 8 x 32 window over a depth segment; one segment once the windows outnumber the blocks
    "roll": Row("roll_plan (biu_conv_roll_rows), nseg = 1", (None, 8, 32), _g_roll, None),
    # first layer on the matrix cores: 3 blocks per CU, one column
    "c1m_fwd3d": Row("biu_c1m_fwd_rows, Geo<3>", (2, 8, 32), _g_c1m, None),
    "c1m_fwd2d": Row("biu_c1m_fwd_rows, Geo<1>", (1, 16, 32), _g_c1m, None),
    "c1m_wgrad3d": Row("biu_c1m_wgrad, Geo<3, HALF>", (1, 8, 32), _g_c1m, None),
    "c1m_wgrad2d": Row("biu_c1m_wgrad, Geo<1, HALF>", (1, 8, 32), _g_c1m, None),
}


def _cdiv(a, b):
    return (a + b - 1) // b


def bricks(row, n, sp):
    """Bricks (items) of a launch of ROWS[row] over n samples of extents sp = (D, H, W) or (H, W)."""
    td, th, tw = ROWS[row].brick
    d, h, w = sp if len(sp) == 3 else (1,) + tuple(sp)
    if row == "wgrad_roll2d":
        n = 1                                        # the batch is the depth axis of one column set
    nbd = 1 if td is None else _cdiv(d, td)
    return n * nbd * _cdiv(h, th) * _cdiv(w, tw)


def grid(row, cus, cols):
    """Blocks per column before the cap at the brick count."""
    return ROWS[row].rule(cus, cols)


def walks(nbricks, g, rounds=3):
    """The precondition of every walking case: `rounds` full rounds plus a ragged last one that at most half of the blocks take."""
    return rounds * g < nbricks and nbricks % g != 0 and nbricks % g <= g / 2


def _extent(nb, t, wide):
    if t == 1:
        return nb
    if wide:                                         # W % 32 == 0 selects the form (tw = 32 there)
        return nb * t
    return nb * t - max(1, t // 3)                    # off the brick, same brick count


def extents(row, g, nd, n=1, depth=None, rounds=3, max_depth=None, min_vox=0):
    """The most compact spatial extents of the first round count whose launch of ROWS[row] with g blocks per column walks: (sp, nbricks) --
    no more bricks than the precondition needs, neighbours along every axis rather than one long row.  depth fixes D where
    an item spans the whole depth; max_depth bounds it where a deeper volume would take another kernel; min_vox: at least so many voxels
    in all (the brick-free bound of a case, see make_case)."""
    r = ROWS[row]
    td, th, tw = r.brick
    per_sample_n = 1 if row == "wgrad_roll2d" else n
    best = None
    for k in range(rounds, rounds + 20):              # (min_vox on a 256-voxel brick: four times the rounds)
        for nb in range(k * g + 1, k * g + g // 2 + 1):
            if nb % per_sample_n:
                continue
            m = nb // per_sample_n
            for a in ([1] if (td is None or nd == 2) else range(1, 65)):
                if m % a:
                    continue
                for b in range(1, 129):
                    if (m // a) % b:
                        continue
                    c = m // a // b
                    d = depth if td is None else _extent(a, td, False)
                    h, w = _extent(b, th, False), _extent(c, tw, r.wide)
                    if nd == 3 and td is not None and (d < 4 or (max_depth and d > max_depth)):
                        continue                      # a volume, not a slab
                    vox = (d or 1) * h * w
                    if n * vox < min_vox:
                        continue
                    key = ((d or 0) + h + w, vox)     # the most compact volume: bricks with neighbours along every axis, then the fewest voxels
                    if best is None or key < best[0]:
                        best = (key, (d, h, w) if nd == 3 else (h, w), nb)
        if best:
            break
    assert best is not None, (row, g, nd, n)
    sp, nb = best[1], best[2]
    assert bricks(row, n, sp) == nb and walks(nb, g, rounds), (row, g, sp, nb)
    return sp, nb


def columns(row, cin, cout, mtl=1):
    """Block columns of a launch of ROWS[row] that reduces over cin channels and writes cout."""
    ntiles = _cdiv(cout, 32)
    if row.startswith("conv16"):
        return cout // (16 * mtl)
    if row in ("conv3d_x3", "conv3d_x6"):
        return ntiles
    if row.startswith("wgrad"):
        return _cdiv(cout, 32) * _cdiv(cin, 32)
    if row.startswith("c1m") or row == "roll":
        return 1
    gy = ntiles // pick_nt(ntiles)
    if row in ("convt3d_fwd", "upconv_fwd"):
        return gy * 8
    if row == "convt2d_fwd":
        return gy * 4
    return gy


Case = namedtuple("Case", "id row nd n cin cout sp cols g nbricks rounds gmac order free")


def make_case(cid, row, cus, nd, cin, cout, *, n=1, depth=None, max_depth=None, rounds=3, cols=None, taps=None, mtl=1, fine=1, api=False):
    """One walking case: (cin, cout) are those of the LAUNCH (a data gradient reduces over the layer's Cout and writes its Cin).  fine: voxels
    of the tensor the reference convolves per voxel of the tensor the launch walks (8 where the bricks lie on the coarse tensor of an
    up-sampling convolution)."""
    cols = cols if cols is not None else columns(row, cin, cout, mtl)
    g = grid(row, cus, cols)
    taps = taps if taps is not None else 3 ** nd
    order = "grouped" if g % 8 == 0 else "plain"
    # Where the launch reports its blocks (api), the case is sized by the brick-free bound -- no brick of any form holds more than 1024 voxels,
    # so ceil(voxels / 1024) >= rounds * blocks walks whatever the brick -- if the float64 reference of that size stays inside the budget;
    # otherwise (and for the launches that report nothing) by the brick of the table.
    for free in ((True, False) if api else (False,)):
        sp, nb = extents(row, g, nd, n=n, depth=depth, rounds=rounds, max_depth=max_depth, min_vox=rounds * g * 1024 if free else 0)
        gmac = n * math.prod(sp) * fine * cin * cout * taps / 1e9
        if gmac <= GMAC_BUDGET:
            break
    return Case(cid, row, nd, n, cin, cout, sp, cols, g, nb, _cdiv(nb, g), gmac, order, free)


# ---------------------------------------------------------------------------------------------------------------
# The walking cases of tests/test_gpu_walk.py.  A spec is static (it parametrises the tests); build(spec, cus) turns it into extents.
#   launch: which launch of the layer cin -> cout the extents make walk -- "fwd" (reduces cin, writes cout), "dgrad" (reduces cout, writes cin:
#   the same kernels with the channel counts swapped), "wgrad" (pairs of 32-wide tiles of dy and x), "wgrad_bn" (its BatchNorm-fused form: the
#   launch of the first x tile, which rewrites da -> dy, walks)
# ---------------------------------------------------------------------------------------------------------------
Spec = namedtuple("Spec", "id family dtype nd cin cout row launch opts")


def _s(id_, family, dtype, nd, cin, cout, row, launch, **opts):
    return Spec(f"{id_}-{dtype}", family, dtype, nd, cin, cout, row, launch, opts)


def _conv_specs():
    out = []
    for dt in ("f32", "bf16"):
        # k_conv_pipe: 16 -> 16 walks forward and backward alike (one column each way); the others walk one way
        out += [
            _s("conv3d-1col-wide", "conv", dt, 3, 16, 16, "conv3d_nt1_wide", "fwd+dgrad"),
            _s("conv3d-1col-narrow", "conv", dt, 3, 16, 16, "conv3d_nt1_narrow", "fwd+dgrad"),
            _s("conv3d-2col", "conv", dt, 3, 16, 112, "conv3d_nt2", "fwd"),
            _s("conv3d-3col", "conv", dt, 3, 16, 80, "conv3d_nt1_narrow", "fwd"),
            _s("conv3d-4col", "conv", dt, 3, 16, 240, "conv3d_nt2", "fwd"),
            _s("dgrad3d-2col", "conv", dt, 3, 112, 16, "conv3d_nt2", "dgrad"),
            _s("dgrad3d-3col", "conv", dt, 3, 80, 16, "conv3d_nt1_wide", "dgrad"),
            _s("dgrad3d-4col", "conv", dt, 3, 240, 16, "conv3d_nt2", "dgrad"),
            _s("conv2d-1col-wide", "conv", dt, 2, 16, 16, "conv2d_nt1_wide", "fwd+dgrad"),
            _s("conv2d-1col-narrow", "conv", dt, 2, 16, 16, "conv2d_nt1_narrow", "fwd+dgrad"),
            _s("conv2d-2col", "conv", dt, 2, 16, 112, "conv2d_nt2_wide", "fwd"),
            _s("conv2d-3col", "conv", dt, 2, 16, 80, "conv2d_nt1_wide", "fwd"),
            _s("conv2d-4col", "conv", dt, 2, 16, 240, "conv2d_nt2_narrow", "fwd"),
            _s("dgrad2d-2col", "conv", dt, 2, 112, 16, "conv2d_nt2_narrow", "dgrad"),
            _s("dgrad2d-3col", "conv", dt, 2, 80, 16, "conv2d_nt1_narrow", "dgrad"),
            _s("dgrad2d-4col", "conv", dt, 2, 240, 16, "conv2d_nt2_wide", "dgrad"),
        ]
    # k_conv16_pipe (bf16): 16 output channels forward, 16 input channels in the data gradient, the two-tile form (Cin = 32, Cout % 32 == 0)
    out += [
        _s("conv16-3d-fwd", "conv", "bf16", 3, 64, 16, "conv16_3d", "fwd"),
        _s("conv16-3d-dgrad", "conv", "bf16", 3, 16, 64, "conv16_3d", "dgrad"),
        _s("conv16-3d-two-tile", "conv", "bf16", 3, 32, 64, "conv16_3d", "fwd", mtl=2),
        _s("conv16-2d-fwd", "conv", "bf16", 2, 32, 16, "conv16_2d", "fwd"),
        _s("conv16-2d-dgrad", "conv", "bf16", 2, 16, 32, "conv16_2d", "dgrad"),
        _s("conv16-2d-two-tile", "conv", "bf16", 2, 32, 64, "conv16_2d", "fwd", mtl=2),
    ]
    # k_conv_roll (bf16, BIU_ROLL=always): 32-row shape forward / 16-row shape backward and the reverse; both directions walk alike
    out += [
        _s("roll-16to32", "roll", "bf16", 3, 16, 32, "roll", "fwd+dgrad", depth=4),
        _s("roll-32to16", "roll", "bf16", 3, 32, 16, "roll", "fwd+dgrad", depth=4),
    ]
    return out


def _split_specs():
    # fp32 3x3x3 as split bf16 products: the mode is latched per process, so these run in a child (tests/walk_probe.py)
    return [
        _s("conv3d-bf16x3", "split", "f32", 3, 16, 80, "conv3d_x3", "fwd", mode=1),
        _s("conv3d-bf16x6", "split", "f32", 3, 16, 80, "conv3d_x6", "fwd", mode=2),
    ]


def _wgrad_specs():
    out = []
    for fam in ("wgrad", "wgrad_bn"):
        out += [
            # (fused: the first x tile's launch has 3 pairs, 85 blocks each -- 64 input channels keep two x tiles inside the reference budget)
            _s(f"{fam}3d-brick", fam, "f32", 3, 96 if fam == "wgrad" else 64, 96, "wgrad3d_f32", fam),
            _s(f"{fam}3d-brick", fam, "bf16", 3, 32, 96, "wgrad3d_bf16", fam, max_depth=7),
            _s(f"{fam}3d-paired-taps", fam, "bf16", 3, 16, 96, "wgrad3d_rr16", fam),
            _s(f"{fam}2d-brick", fam, "f32", 2, 96, 96, "wgrad2d_f32", fam),
            _s(f"{fam}2d-brick", fam, "bf16", 2, 96, 96, "wgrad2d_bf16", fam, n=2),
            # (plain: four pairs of half-filled tiles; fused: one x tile, so that a single launch of two pairs both rewrites da and walks)
            _s(f"{fam}3d-roll", fam, "bf16", 3, 48 if fam == "wgrad" else 24, 48, "wgrad_roll3d", fam, depth=8),
            _s(f"{fam}3d-roll-16ch", fam, "bf16", 3, 32, 16, "wgrad_roll3d", fam, depth=8),
            _s(f"{fam}2d-roll", fam, "bf16", 2, 48, 48, "wgrad_roll2d", fam, n=8),
        ]
    return out


def _convt_specs():
    out = []
    for dt in ("f32", "bf16"):
        # 16 input channels keep bf16 off k_convt_all (it takes multiples of 32 up to 64); bricks lie on the coarse tensor
        out += [
            _s("convt3d-fwd-8col", "convt", dt, 3, 16, 32, "convt3d_fwd", "fwd"),
            _s("convt3d-fwd-24col", "convt", dt, 3, 16, 96, "convt3d_fwd", "fwd"),
            _s("convt2d-fwd-4col", "convt", dt, 2, 16, 32, "convt2d_fwd", "fwd"),
            _s("convt3d-dgrad-2col", "convt", dt, 3, 112, 16, "convt3d_dgrad", "dgrad"),
            _s("convt3d-dgrad-3col", "convt", dt, 3, 96, 16, "convt3d_dgrad", "dgrad"),
            _s("convt2d-dgrad-2col", "convt", dt, 2, 128, 16, "convt2d_dgrad", "dgrad"),
        ]
    return out


def _upconv_specs():
    out = []
    for dt in ("f32", "bf16"):
        out += [
            _s("upconv-fwd-8col", "upconv", dt, 3, 16, 32, "upconv_fwd", "fwd"),
            _s("upconv-fwd-24col", "upconv", dt, 3, 16, 96, "upconv_fwd", "fwd"),
            # the data gradient onto the coarse tensor (reduces dy's 32 channels, writes 16: one column); its reference is the folded one
            # (upconv_folded_ref below, 8 taps on the coarse tensor per parity class instead of 27 on the fine one)
            _s("upconv-dgrad-1col", "upconv", dt, 3, 16, 32, "upconv_dgrad", "dgrad"),
        ]
    # biu_upconv_bwd_weight_bn: one dy tile per block, and two (dy wider than 32 channels: half the columns)
    out += [
        _s("upconv-wgrad-1tile", "upconv_wgrad", "f32", 3, 16, 32, "upconv_wgrad_f32", "wgrad_bn"),
        _s("upconv-wgrad-2tile", "upconv_wgrad", "f32", 3, 16, 96, "upconv_wgrad_f32", "wgrad_bn"),
        # (bf16: 512-voxel bricks, twice the fp32 case's voxels -- 16 dy channels, a half-filled tile, keep its fine tensors at 45 M elements)
        _s("upconv-wgrad-1tile", "upconv_wgrad", "bf16", 3, 16, 16, "upconv_wgrad_bf16", "wgrad_bn"),
    ]
    return out


def _foldt_specs():
    # ConvTranspose + concat + conv of a decoder level in its brick form (a 16-channel skip keeps bf16 off the rolling-window form): the up
    # half's launch on the coarse tensor, eight parity columns, walks.  cin = cup + cskip: what the reference's 3x3x3 convolution reduces.
    return [_s("foldt-brick-form", "foldt", dt, 3, 32, 32, "upconv_fwd", "fwd", cl=32, cup=16, cs=16) for dt in ("f32", "bf16")]


def _rank1_specs():
    # biu_conv_bwd_weight_bn_rank1: k_wgrad_roll's fused 16-channel form with da rebuilt from a one-channel head's gradient
    return [_s("rank1-16ch", "rank1", "bf16", 3, 32, 16, "wgrad_roll3d", "wgrad_bn", depth=8)]


def _cat_specs():
    # two-source forms (x = concat(x0: 64, x1: 32 channels) without a concat buffer; biu_conv_cat_ok: the first source ends on a tile boundary
    # of the data gradient, so 64 + 32 are the fewest channels).  Forward: 16 output channels, one column of 1024-voxel bricks, 10.9 GMAC in
    # 2-D.  On bf16 the two-source call stays on k_conv_pipe there (biu_mfma_conv keeps a second source off k_conv16_pipe) while the
    # concat-buffer call the helper also makes takes k_conv16_pipe: the helper compares the two with a tolerance instead of bit for bit.
    # A walking 3-D forward is past the budget in either type: the same bricks with 27 taps = 32.6 GMAC.
    # The 3-D data gradient (reduces 16 channels, writes 96 in three columns: 10 GMAC) and weight gradient (9 pairs of tiles) fit.
    out = [_s("cat2d-fwd-1col", "cat", "f32", 2, 96, 16, "conv2d_nt1_wide", "fwd"),
           _s("cat2d-fwd-1col", "cat", "bf16", 2, 96, 16, "conv2d_nt1_wide", "fwd"),
           _s("cat3d-dgrad-3col", "cat", "f32", 3, 96, 16, "conv3d_nt1_narrow", "dgrad")]
    for dt in ("f32", "bf16"):
        out += [
            _s("cat2d-dgrad-3col", "cat", dt, 2, 96, 48, "conv2d_nt1_narrow", "dgrad"),
            _s("cat2d-wgrad", "cat", dt, 2, 96, 48, "wgrad2d_f32" if dt == "f32" else "wgrad2d_bf16", "wgrad"),
            _s("cat3d-wgrad", "cat", dt, 3, 96, 96, "wgrad3d_f32" if dt == "f32" else "wgrad3d_bf16", "wgrad", **({} if dt == "f32" else {"max_depth": 7})),
        ]
    return out


def _c1m_specs():
    # first layer on the matrix cores (bf16, one input channel): 48 output channels = a 32- and a 16-channel launch; two rounds are enough
    return [
        _s("c1m-3d-fwd", "c1m", "bf16", 3, 1, 48, "c1m_fwd3d", "fwd", rounds=2),
        _s("c1m-2d-fwd", "c1m", "bf16", 2, 1, 48, "c1m_fwd2d", "fwd", rounds=2),
        _s("c1m-3d-wgrad", "c1m", "bf16", 3, 1, 48, "c1m_wgrad3d", "wgrad_bn", rounds=2),
        _s("c1m-2d-wgrad", "c1m", "bf16", 2, 1, 48, "c1m_wgrad2d", "wgrad_bn", rounds=2),
    ]


SPECS = _conv_specs() + _split_specs() + _wgrad_specs() + _cat_specs() + _convt_specs() + _upconv_specs() + _foldt_specs() + _rank1_specs() + _c1m_specs()
SPEC_BY_ID = {s.id: s for s in SPECS}
assert len(SPEC_BY_ID) == len(SPECS)


def build(spec, cus):
    """The extents of a spec on a device with `cus` compute units."""
    o = spec.opts
    kw = dict(n=o.get("n", 1), depth=o.get("depth"), max_depth=o.get("max_depth"), rounds=o.get("rounds", 3), mtl=o.get("mtl", 1))
    if spec.launch == "dgrad":
        cin, cout = spec.cout, spec.cin                                   # the launch reduces over the layer's output channels
    else:
        cin, cout = spec.cin, spec.cout
    if spec.launch == "wgrad_bn" and not spec.row.startswith("c1m"):
        kw["cols"] = _cdiv(spec.cout, 32)                                 # the launch of the first x tile (pairs = dy tiles) rewrites da -> dy
    if spec.family == "convt":
        kw["taps"] = 2 ** spec.nd                                         # per coarse voxel: 2^nd fine voxels of one tap each
    if spec.family in ("upconv", "upconv_wgrad", "foldt"):
        kw["fine"] = 8
    if spec.family == "upconv_wgrad":
        kw["cols"] = _cdiv(spec.cout, 64 if spec.cout > 32 else 32)       # two dy tiles per block once dy has them; one x tile
    if spec.family == "upconv_wgrad" or (spec.family == "upconv" and spec.launch == "dgrad"):
        kw["taps"] = 8                                                    # the folded reference: 2 x 2 x 2 taps on the coarse tensor per parity class
    kw["api"] = api_reports_rows(spec)
    return make_case(spec.id, spec.row, cus, spec.nd, cin, cout, **kw)


def api_reports_rows(spec):
    """Does the entry point whose launch the spec makes walk hand out its blocks per column (bn_nblk / nblk)?  The forward calls with
    statistics and the data gradients with the BatchNorm-backward sums do; biu_convt_fwd, biu_upconv_bwd_data, biu_conv_bwd_data_cat and every
    weight gradient do not."""
    if spec.launch in ("wgrad", "wgrad_bn"):
        return False
    if spec.launch == "dgrad":
        return spec.family in ("conv", "roll", "convt")
    return spec.family != "convt"


def check_case(c, rounds=3):
    """Every condition of a generated case (tests/test_walk_geometry_host.py; the GPU tests assert them again from what the launch reports)."""
    r = ROWS[c.row]
    assert walks(c.nbricks, c.g, rounds), c
    assert bricks(c.row, c.n, c.sp) == c.nbricks, c
    td, th, tw = r.brick
    d, h, w = c.sp if c.nd == 3 else (1,) + tuple(c.sp)
    assert h % th != 0, c
    assert (w % 32 == 0) if r.wide else (w % tw != 0), c
    if r.wide is False:
        assert w % 32 != 0, c
    if td not in (None, 1):
        assert d % td != 0, c
    assert c.gmac <= GMAC_BUDGET, c
    return True


def upconv_folded_ref(x, w, b=None):
    """F.conv3d(F.interpolate(x, scale_factor=2, mode='nearest'), w, b, padding=1) at 8 taps per output voxel instead of 27, in torch: the fine
    voxel 2v + p reads, along each axis, the coarse voxels v - 1 and v (p = 0; fine tap 0 | taps 1, 2) or v and v + 1 (p = 1; taps 0, 1 | tap 2).
    So every parity class is a 2 x 2 x 2 convolution of the coarse tensor, padded by one voxel on the side it reaches over, with the fine taps
    that read the same coarse voxel summed.  Differentiable: autograd gives the data and the weight gradient at the same cost
    (tests/test_walk_geometry_host.py holds it against the unfolded expression)."""
    import torch
    import torch.nn.functional as F
    n, _, d, h, wd = x.shape
    y = x.new_empty(n, w.shape[0], 2 * d, 2 * h, 2 * wd)
    groups = (((0,), (1, 2)), ((0, 1), (2,)))                                # [parity][coarse tap] -> fine taps
    for p in range(8):
        par = (p >> 2 & 1, p >> 1 & 1, p & 1)
        wf = w
        for ax, pa in enumerate(par):                                        # fold one axis after the other: 3 taps -> 2
            wf = torch.stack([wf.index_select(2 + ax, torch.tensor(g)).sum(2 + ax) for g in groups[pa]], 2 + ax)
        pad = [v for pa in reversed(par) for v in ((1, 0) if pa == 0 else (0, 1))]      # F.pad: last axis first
        y[:, :, par[0]::2, par[1]::2, par[2]::2] = F.conv3d(F.pad(x, pad), wf, b)
    return y
