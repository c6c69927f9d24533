"""The arithmetic facts the uint8 widening of ``biu_from_nchw_u8`` / ``biu_u8_to_f32`` rests on, pinned on the host with numpy float32
(IEEE single, round to nearest even -- what the device's correctly rounded fp32 division gives too).

The reference's data contract is the QUOTIENT ``tile.astype('float32') / 255`` (``unet3d/predict.py:162``, ``unet3d/data.py:251-255``,
``siam_unet/predict.py:206``), which ``TileStore.__getitem__`` and the augmentation kernels' loads compute as well.  The PRODUCT with the
fp32-rounded reciprocal, ``float32(k) * float32(1 / 255)``, is a different function of the byte."""
import numpy as np

K = np.arange(256, dtype=np.uint8)
QUOT = K.astype(np.float32) / np.float32(255)
PROD = K.astype(np.float32) * np.float32(1.0 / 255.0)


def to_bf16_bits(x):
    """Round-to-nearest-even bf16 of finite float32 values, as the upper 16 bits."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def test_quotient_and_product_differ_for_126_codes():
    assert QUOT.dtype == PROD.dtype == np.float32
    differ = np.flatnonzero(QUOT != PROD)
    assert len(differ) == 126
    assert differ[:8].tolist() == [3, 6, 7, 12, 13, 14, 15, 24]
    # never by more than the last bit
    assert int(np.abs(QUOT.view(np.int32).astype(np.int64) - PROD.view(np.int32).astype(np.int64)).max()) == 1


def test_quotient_is_the_correctly_rounded_value():
    exact = K.astype(np.float64) / 255.0                     # 8-bit / 8-bit: the float64 quotient is far closer than half an fp32 ulp
    assert np.array_equal(QUOT, exact.astype(np.float32))
    assert QUOT[0] == 0.0 and QUOT[255] == 1.0               # binary masks (0 / 255) become exactly 0 and 1


def test_none_differ_after_rounding_to_bf16():
    assert np.array_equal(to_bf16_bits(QUOT), to_bf16_bits(PROD))


def test_quantising_the_quotient_returns_the_code():
    """``(p * 255).astype('uint8')`` (truncation, unet/predict.py:200) of the quotient is the byte again: the uint8 round trip
    through the float contract is lossless."""
    assert np.array_equal((QUOT * np.float32(255)).astype(np.uint8), K)


def test_tile_store_item_is_the_quotient(tmp_path):
    from bio_image_unet_amd.feed import TileStore
    st = TileStore.create(str(tmp_path / "s"), 1, {"image": (16, 16)})
    st.maps["image"][0] = K.reshape(16, 16)
    st.flush()
    item = st[0]["image"].numpy()
    assert item.dtype == np.float32 and np.array_equal(item.view(np.uint32), QUOT.reshape(16, 16).view(np.uint32))
