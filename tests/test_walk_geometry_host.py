"""tests/walk_geometry.py on the CPU: for the CU counts of an MI355X (256), an MI300X (304) and a small part (64) every generated shape makes
its launch walk -- three full rounds (two for the first layer) plus a ragged last one that at most half of the blocks take -- with extents
off the brick, inside the budget of the float64 reference; and the grid rule mirrors the launch functions' on the values they document."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import walk_geometry as G

CUS = [256, 304, 64]


def test_grid_per_column_matches_the_documented_values():
    # biu_conv_mfma.hip: "3 columns: 85 blocks each, not 80"; a 96 -> 96 weight gradient: 9 pairs, 28 blocks each
    assert G.grid_per_column(256, 1) == 256 and G.grid_per_column(256, 2) == 128 and G.grid_per_column(256, 4) == 64
    assert G.grid_per_column(256, 3) == 85
    assert G.grid_per_column(256, 8) == 32 and G.grid_per_column(256, 16) == 16
    assert G.grid("wgrad3d_f32", 256, 9) == 28
    assert G.grid("c1m_fwd3d", 256, 1) == 768
    assert G.grid_per_column(64, 16) == 8                                  # never under 8 blocks per column
    assert G.pick_nt(1) == 1 and G.pick_nt(3) == 1 and G.pick_nt(4) == 2 and G.pick_nt(8) == 2


def test_walk_orders_of_the_column_counts_on_256_cus():
    order = {cols: ("grouped" if G.grid_per_column(256, cols) % 8 == 0 else "plain") for cols in (1, 2, 3, 4)}
    assert order == {1: "grouped", 2: "grouped", 3: "plain", 4: "grouped"}
    # every k_conv_pipe column count of the issue is a case, in 2-D and 3-D
    for nd in (2, 3):
        got = {G.build(s, 256).cols for s in G.SPECS if s.family == "conv" and s.nd == nd and s.row.startswith("conv%dd" % nd) and "fwd" in s.launch}
        assert got == {1, 2, 3, 4}, (nd, got)


@pytest.mark.parametrize("cus", CUS)
def test_every_generated_shape_walks_and_fits_the_budget(cus):
    for spec in G.SPECS:
        c = G.build(spec, cus)
        rounds = spec.opts.get("rounds", 3)
        assert G.check_case(c, rounds)
        assert c.rounds >= rounds + 1                                       # a first, a middle (except the first layer) and a last item
        assert c.g < c.nbricks
        if c.free:                                                          # the brick-free bound the GPU test asserts from the reported rows
            assert -(-c.n * math.prod(c.sp) // 1024) >= rounds * c.g
        assert not c.free or G.api_reports_rows(spec)
        if spec.launch in ("wgrad", "wgrad_bn") and not spec.row.startswith("c1m"):
            # every launch of the weight gradient walks at least three rounds: the plain one over all pairs, the fused one over the first x
            # tile's pairs and then over the others'
            nit, njt = -(-spec.cout // 32), -(-spec.cin // 32)
            launches = [nit * njt] if spec.launch == "wgrad" or njt == 1 else [nit, nit * (njt - 1)]
            for pairs in launches:
                assert 3 * G.grid(c.row, cus, pairs) < c.nbricks, (spec.id, pairs)


def test_the_brick_free_bound_is_taken_wherever_it_fits_the_budget():
    """k_conv_pipe on 256 CUs: every 2-D case and the 1- and 3-column 3-D cases (1024-voxel bricks: 5.4 and 9 GMAC) are sized so that the GPU
    test can assert ceil(voxels / 1024) >= 3 * rows from the reported rows alone; the 2- and 4-column 3-D cases (512-voxel bricks: 17-19 GMAC
    at that size) are counted with the table's brick."""
    for s in G.SPECS:
        if s.family == "conv" and s.row.startswith("conv") and not s.row.startswith("conv16"):
            c = G.build(s, 256)
            assert c.free == (s.nd == 2 or c.cols in (1, 3)), (s.id, c)


def test_rows_name_the_launch_they_mirror():
    for name, r in G.ROWS.items():
        assert r.mirrors and len(r.brick) == 3, name
    assert {s.row for s in G.SPECS} <= set(G.ROWS)


def test_the_folded_reference_is_upsample_then_conv():
    """upconv_folded_ref (8 taps per parity class on the coarse tensor) == nearest x2 + Conv3d(k3, padding=1) in float64, values and both
    gradients, on extents that are odd and as small as one voxel."""
    for shape in ((2, 3, 3, 5, 4), (1, 2, 1, 1, 7)):
        g = torch.Generator().manual_seed(0)
        x = torch.randn(*shape, dtype=torch.float64, generator=g).requires_grad_(True)
        w = torch.randn(5, shape[1], 3, 3, 3, dtype=torch.float64, generator=g).requires_grad_(True)
        b = torch.randn(5, dtype=torch.float64, generator=g)
        want = F.conv3d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
        got = G.upconv_folded_ref(x, w, b)
        dy = torch.randn(*want.shape, dtype=torch.float64, generator=g)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
        for a_, b_ in zip(torch.autograd.grad(got, (x, w), dy), torch.autograd.grad(want, (x, w), dy)):
            torch.testing.assert_close(a_, b_, rtol=1e-12, atol=1e-12)
