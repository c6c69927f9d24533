"""What the per-product probes of the split fp32 product modes share (tests/fp32_product_probe.py on the GPU, tests/test_fp32_split_host.py on the
CPU): the operand generator, a torch restatement of the kernels' split product, and the bounds both are held to.  Kept in ONE module so that
the statement "a product with a missing term exceeds the bound" is proven on the very operands the GPU probe multiplies.

The kernels (bio_image_unet_amd/csrc/biu_conv_mfma.hip): split_bf16 rounds a value to bf16 (nearest even), subtracts (exact in fp32) and
repeats -- hi, lo for bf16x3, hi, mid, lo for bf16x6 --; a product is the terms part a of one operand x part b of the other with a + b < parts,
the activation's smallest part first, each an exact bf16 x bf16 product added to an fp32 accumulator."""
import torch

# relative error a single product may have: 2^-22 bf16x6 and 2^-14 bf16x3 -- the c of tests/test_gpu_fp32_products_3d.py: twice the 2^-23 / 2^-15
# that the dropped terms and the split's own rounding leave (the rest is for the matrix pipe's fp32 accumulation of the terms: measured worst
# 2^-22.6 / 2^-15.2) --, and an fp32 product's own rounding to nearest (2^-24) times two for the exact fp32 MFMA
BOUND = {"exact": 2.0 ** -23, "bf16x3": 2.0 ** -14, "bf16x6": 2.0 ** -22}
PARTS = {"bf16x3": 2, "bf16x6": 3}
# the smallest number of single products a probed launch yields (the GPU test asserts it; the CPU test draws this many pairs)
MIN_PRODUCTS = 4096


def operands(*shape, seed):
    """Full-mantissa fp32 values with |v| in [0.25, 4): a random sign, one of the four binades 2^-2 .. 2^1 and 23 random mantissa bits."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    mant = torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int64)
    expo = torch.randint(125, 129, (n,), generator=g, dtype=torch.int64)          # biased exponent: 125 = 2^-2
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64)
    bits = (sign << 31) | (expo << 23) | mant
    bits = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32).reshape(shape).clone()


def split_bf16(v, parts):
    """[hi, (mid,) lo] as fp32 tensors: round to bf16 (nearest even), subtract (exact in fp32), repeat."""
    out, r = [], v.clone()
    for _ in range(parts):
        p = r.bfloat16().float()
        out.append(p)
        r = r - p
    return out


def terms(parts):
    """(a, b) part pairs in the order the kernels issue them: the second operand's smallest part first."""
    return [(ka, kb) for kb in range(parts - 1, -1, -1) for ka in range(parts - 1 - kb, -1, -1)]


def split_product(a, b, parts, drop=None):
    """The kernels' product of fp32 tensors a, b; `drop` = one (a part, b part) pair left out."""
    pa, pb = split_bf16(a, parts), split_bf16(b, parts)
    acc = torch.zeros_like(a)
    for ka, kb in terms(parts):
        if (ka, kb) != drop:
            acc = acc + pa[ka] * pb[kb]          # bf16 x bf16 is exact in fp32; the sum rounds to nearest
    return acc


def rel_err(got, a, b):
    """|got - a b| / |a b| against the float64 product of the fp32 values (exact: 48 significant bits)."""
    ref = a.double() * b.double()
    return (got.double() - ref).abs() / ref.abs()
