"""The source-side swizzle of the LDS-DMA staged x.Wx launch (csrc/air_gemm_bf16.hip, gemm_xwx_glds_kernel), in pure
Python against the formulas of the kernels.

Register staging (store_images) puts the 16-byte piece (image c, row, slot g of 8 k) at ImgA[(c*16 + row)*64 +
((g ^ (row & 7)) << 3)].  An LDS-DMA instruction cannot choose its destination -- lane l of a wave writes at the wave's
base + 16 l -- so the piece WRITTEN at linear index u = (c, row, slot p) has to FETCH slot p ^ (row & 7) of its row.
The two images must be the same for every (row, slot), the fetch order must be a permutation of the eight slots of one
128-byte line, and the per-thread quantities the kernel precomputes must describe exactly that map."""

KB, BM, THREADS = 64, 16, 256


def _register_image(R):
    """position (in 16-byte slots) -> (image, row, source slot) as store_images lays it out"""
    img = {}
    for c in range(R):
        for row in range(BM):
            for g in range(8):
                pos = ((c * BM + row) * KB + ((g ^ (row & 7)) << 3)) // 8
                assert pos not in img
                img[pos] = (c, row, g)
    return img


def _dma_image(R):
    """the same map as the LDS-DMA kernel produces it: thread tid, pass i -> linear piece u -> fetched (image, row, slot)"""
    img = {}
    for i in range(R * BM * 8 // THREADS):
        for tid in range(THREADS):
            lane, wave = tid & 63, tid >> 6
            arow = (tid >> 3) & 15
            asg = (tid & 7) ^ (arow & 7)
            ka = (tid >> 7) * KB + asg * 8                 # k within the pass (two images)
            k = 2 * KB * i + ka
            dest = wave * 1024 + THREADS * 16 * i + lane * 16   # wave-uniform base + lane * 16
            u = tid + THREADS * i
            assert dest == u * 16
            assert dest // 16 not in img
            img[dest // 16] = (k // KB, arow, (k % KB) // 8)
    return img


def test_source_swizzle_is_a_permutation_within_each_128_byte_row():
    for row in range(BM):
        fetched = [g ^ (row & 7) for g in range(8)]
        assert sorted(fetched) == list(range(8))
        # an involution: the fragment read applies the same XOR to find logical slot s again
        assert [fetched[f] for f in fetched] == list(range(8))
        # every fetch stays inside the row's own 128-byte line
        assert all(0 <= 16 * f < 128 for f in fetched)


def test_dma_image_equals_the_register_staged_image_for_all_rows_and_slots():
    for R in (16, 40):
        reg, dma = _register_image(R), _dma_image(R)
        assert len(reg) == len(dma) == R * BM * 8
        assert reg == dma


def test_fragment_read_finds_logical_slot_in_both_images():
    # the MFMA loop reads logical slot s of (c, row) at ((c*16 + row)*64 + ((s ^ (row & 7)) << 3))
    dma = _dma_image(40)
    for c in (0, 17, 39):
        for row in range(BM):
            for s in range(8):
                pos = ((c * BM + row) * KB + ((s ^ (row & 7)) << 3)) // 8
                assert dma[pos] == (c, row, s)


def test_b_panel_image_is_lane_linear():
    # piece t of a pass: 16 bytes = two gates of one k; destination 16 t, source 16 t of the contiguous panel block
    for i in range(3):
        for tid in range(THREADS):
            t = tid + THREADS * i
            k = 2 * KB * i + (tid >> 1)
            assert t * 16 == k * 32 + (tid & 1) * 16
            assert (tid >> 6) * 1024 + THREADS * 16 * i + (tid & 63) * 16 == t * 16
