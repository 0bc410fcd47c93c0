"""mask_layout.py against include/placement.h's sentences: word indices worked by hand at the sizes where the
roundings bite, the round trip, the coverage of every extent, and the extents against the engine's allocation."""
import numpy as np
import pytest

import mask_layout as ML

SIZES_S = [1, 255, 256, 257, 500, 1024, 1025, 8193]
SIZES_J = [1, 16, 17, 64, 65, 257]


def pitches(S):
    """The pitches the two row-major paths report: whole 8192-node blocks, and 2048 W-node blocks, W = 1, 2, 4."""
    return sorted({-(-S // 8192) * 128} | {-(-S // (2048 * W)) * 32 * W for W in (1, 2, 4)})


# (layout, J, S, pitch, (row, col), index): row = j or b, col = c or n -- each worked from the header's sentence
BY_HAND = [
    # tiles: ((j / 16) * Wt + c / 4) * 64 + (j % 16) * 4 + c % 4
    (ML.NODE_TILES, 1, 1, 0, (0, 0), 0),                  # Wn 1, Wt 1
    (ML.NODE_TILES, 16, 255, 0, (15, 3), 63),             # Wn 4, Wt 1: the last word of the first tile
    (ML.NODE_TILES, 17, 256, 0, (16, 3), 67),             # Wt 1: band 1 starts at 64
    (ML.NODE_TILES, 17, 257, 0, (0, 4), 64),              # Wn 5, Wt 2: the fifth word opens tile column 1
    (ML.NODE_TILES, 17, 257, 0, (16, 0), 128),            # band 1 starts at Wt * 64
    (ML.NODE_TILES, 17, 257, 0, (16, 4), 192),
    (ML.NODE_TILES, 65, 500, 0, (64, 7), (4 * 2 + 1) * 64 + 3),          # Wn 8, Wt 2
    (ML.NODE_TILES, 64, 1024, 0, (63, 15), (3 * 4 + 3) * 64 + 15 * 4 + 3),   # Wn 16, Wt 4: the last word of all
    (ML.NODE_TILES, 257, 1025, 0, (33, 16), (2 * 5 + 4) * 64 + 4),       # Wn 17, Wt 5
    (ML.NODE_TILES, 257, 8193, 0, (256, 128), (16 * 33 + 32) * 64),      # Wn 129, Wt 33
    # job bits: b * St + n, St = S rounded up to 1024
    (ML.JOB_BITS, 1, 1, 0, (0, 0), 0),
    (ML.JOB_BITS, 65, 255, 0, (1, 254), 1024 + 254),
    (ML.JOB_BITS, 65, 500, 0, (1, 0), 1024),              # rounded up to 512 this word would sit at 512
    (ML.JOB_BITS, 65, 500, 0, (1, 499), 1523),
    (ML.JOB_BITS, 64, 1024, 0, (0, 1023), 1023),
    (ML.JOB_BITS, 65, 1024, 0, (1, 0), 1024),
    (ML.JOB_BITS, 65, 1025, 0, (1, 1024), 2048 + 1024),
    (ML.JOB_BITS, 257, 8193, 0, (4, 8192), 4 * 9216 + 8192),
    # node blocks: ((c / 128) * J + j) * 128 + c % 128
    (ML.NODE_BLOCKS, 17, 257, 0, (2, 4), 260),
    (ML.NODE_BLOCKS, 17, 8193, 0, (16, 127), 16 * 128 + 127),
    (ML.NODE_BLOCKS, 17, 8193, 0, (3, 128), (17 + 3) * 128),
    (ML.NODE_BLOCKS, 257, 8193, 0, (256, 128), (257 + 256) * 128),
    (ML.NODE_BLOCKS, 1, 1, 0, (0, 0), 0),
    # rows: j * P + c
    (ML.ROWS, 65, 1025, 128, (64, 16), 64 * 128 + 16),
    (ML.ROWS, 65, 2049, 64, (64, 32), 64 * 64 + 32),
    (ML.ROWS, 17, 8193, 256, (16, 128), 16 * 256 + 128),
    (ML.ROWS, 16, 500, 32, (1, 0), 32),
]


@pytest.mark.parametrize("layout,J,S,pitch,pos,want", BY_HAND)
def test_word_index_by_hand(layout, J, S, pitch, pos, want):
    idx = ML.word_index(layout, J, S, pitch)
    assert idx[pos] == want
    assert want < ML.extent(layout, J, S, pitch)


def test_extents_by_hand():
    assert ML.extent(ML.NODE_TILES, 1, 1) == 64                    # one tile
    assert ML.extent(ML.NODE_TILES, 17, 257) == 2 * 2 * 64
    assert ML.extent(ML.NODE_TILES, 257, 8193) == 17 * 33 * 64
    assert ML.extent(ML.JOB_BITS, 65, 500) == 2 * 1024
    assert ML.extent(ML.JOB_BITS, 64, 1025) == 2048
    assert ML.extent(ML.JOB_BITS, 257, 8193) == 5 * 9216
    assert ML.extent(ML.NODE_BLOCKS, 17, 8192) == 17 * 128
    assert ML.extent(ML.NODE_BLOCKS, 17, 8193) == 2 * 17 * 128
    assert ML.extent(ML.ROWS, 65, 2049, 64) == 65 * 64
    assert ML.job_bits_stride(1) == ML.job_bits_stride(1024) == 1024 and ML.job_bits_stride(1025) == 2048


def test_job_bits_word_holds_the_jobs_of_a_node():
    """Bit j % 64 of word (j / 64, n) is fit(j, n)."""
    J, S = 130, 70
    rows = np.zeros((J, 2), dtype=np.uint64)
    rows[0, 0] = 1                       # (job 0, node 0)
    rows[65, 1] = np.uint64(1) << np.uint64(5)      # (job 65, node 69)
    rows[129, 0] = np.uint64(1) << np.uint64(63)    # (job 129, node 63)
    img = ML.image(rows, ML.JOB_BITS, J, S)
    want = np.zeros(3 * 1024, dtype=np.uint64)
    want[0] = 1
    want[1024 + 69] = 2                  # job 65 = band 1, bit 1
    want[2048 + 63] = 2                  # job 129 = band 2, bit 1
    np.testing.assert_array_equal(img, want)


def random_rows(rng, J, S):
    Wn = ML.words_per_row(S)
    rows = rng.integers(0, 1 << 63, (J, Wn), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (J, Wn), dtype=np.uint64)
    if S % 64:
        rows[:, -1] &= np.uint64((1 << (S % 64)) - 1)
    return rows


@pytest.mark.parametrize("S", SIZES_S)
@pytest.mark.parametrize("J", SIZES_J)
def test_round_trip_and_coverage(J, S):
    rng = np.random.default_rng(1000 * J + S)
    rows = random_rows(rng, J, S)
    for layout in ML.LAYOUTS:
        for pitch in (pitches(S) if layout == ML.ROWS else [0]):
            n = ML.extent(layout, J, S, pitch)
            img = ML.image(rows, layout, J, S, pitch)
            assert img.shape == (n,) and img.dtype == np.uint64
            np.testing.assert_array_equal(ML.rows_of(img, layout, J, S, pitch), rows)
            # every word of the extent is addressed by exactly one (j, c) / (b, n), or is padding (zero)
            idx = ML.word_index(layout, J, S, pitch).reshape(-1)
            assert idx.min() >= 0 and idx.max() < n
            assert len(np.unique(idx)) == len(idx)
            pad = np.ones(n, dtype=bool)
            pad[idx] = False
            assert not img[pad].any()
            # the bits set are the mask's, no more: padding bits inside addressed words are zero too
            assert np.unpackbits(img.view(np.uint8)).sum() == np.unpackbits(rows.view(np.uint8)).sum()
            # bits past the last node in a row's last word do not reach the image
            dirty = rows.copy()
            if S % 64:
                dirty[:, -1] |= ~np.uint64((1 << (S % 64)) - 1)
            np.testing.assert_array_equal(ML.image(dirty, layout, J, S, pitch), img)
            # what is left unspecified never holds a valid pair
            assert not ML.unspecified(layout, J, S, pitch)[idx].any()
            if layout != ML.NODE_TILES:
                assert not ML.unspecified(layout, J, S, pitch).any()


def test_unspecified_is_the_tile_rows_past_the_last_job():
    J, S = 17, 257                                   # Wt 2: band 1 holds job 16 and fifteen padding rows
    u = ML.unspecified(ML.NODE_TILES, J, S)
    assert u.sum() == 15 * 8 and not u[:128].any()
    assert not u[128:132].any() and u[132:192].all()             # tile (1, 0): row 16, then rows 17 .. 31
    assert not u[192:196].any() and u[196:256].all()
    assert not ML.unspecified(ML.NODE_TILES, 16, S).any()


def round_up(a, b):
    return -(-a // b) * b


@pytest.mark.parametrize("S", SIZES_S + [2049, 16385])
@pytest.mark.parametrize("J", SIZES_J)
def test_extents_fit_the_allocation(J, S):
    """The words fit_upload allocates (pe_engine.cpp: `mask_words` in fit_upload, with Jp = round_up(J, FM_JT = 256)
    of fit_upload, code_Jp = round_up(J, 64) and node_stride = round_up(Ns, 64 * FC_CH = 1024) of build_codes, pl_nblk =
    ceil(Ns / 8192) and pl_pitch >= pl_nblk of build_planes, lds_pitch = ceil(Ns / (2048 W)) * 2048 W / 64 of
    build_lds), restated as plain arithmetic: no extent passes them."""
    Wn = -(-S // 64)
    Wt = -(-Wn // 4)
    alloc_tiles = round_up(max(J, 1), 256) * max(Wt, 1) * 4
    alloc_coded = round_up(J, 64) // 64 * round_up(max(S, 1), 1024)
    nblk = -(-max(S, 1) // 8192)
    alloc_blocks = max(J, 1) * nblk * 128
    assert ML.extent(ML.NODE_TILES, J, S) <= alloc_tiles
    assert ML.extent(ML.JOB_BITS, J, S) <= alloc_coded
    assert ML.extent(ML.NODE_BLOCKS, J, S) <= alloc_blocks
    pitch_planes = nblk * 128
    assert ML.extent(ML.ROWS, J, S, pitch_planes) <= max(J, 1) * nblk * 128
    ML.check_pitch(S, pitch_planes, True)
    for W in (1, 2, 4):
        lds_pitch = -(-S // (2048 * W)) * 2048 * W // 64
        assert ML.extent(ML.ROWS, J, S, lds_pitch) <= max(J, 1) * lds_pitch
        ML.check_pitch(S, lds_pitch, False)


def test_check_pitch_refuses():
    with pytest.raises(AssertionError):
        ML.check_pitch(2049, 32, False)       # below words_per_row
    with pytest.raises(AssertionError):
        ML.check_pitch(100, 8, False)         # half a line
    with pytest.raises(AssertionError):
        ML.check_pitch(2049, 64, True)        # no whole 8192-node block
    ML.check_pitch(2049, 64, False)
