"""The four device layouts of the fit mask, restated from the text of include/placement.h in plain numpy: no
engine, no kernel header.  A consumer on the device has nothing but those sentences, so the tests index the raw
device words (Engine.read_mask_words) with the formulas written here and never with the engine's own gather.

J jobs, S shard nodes, Wn = ceil(S / 64) words per row, Wt = ceil(Wn / 4).

    PE_MASK_NODE_TILES   word (j, c) at ((j / 16) * Wt + c / 4) * 64 + (j % 16) * 4 + c % 4
    PE_MASK_JOB_BITS     word (b, n), jobs 64b .. 64b + 63 of node n (bit j % 64), at b * St + n,
                         St = S rounded up to 1024
    PE_MASK_NODE_BLOCKS  word (j, c) at ((c / 128) * J + j) * 128 + c % 128
    PE_MASK_ROWS         word (j, c) at j * P + c, P = pe_fit_mask_row_pitch

    extent(layout, J, S, pitch)        the words those formulas address
    image(rows, layout, J, S, pitch)   the whole expected device image of a row-major [J][Wn] mask: zero wherever
                                       a word or bit belongs to no valid (job, node) pair
    rows_of(img, layout, J, S, pitch)  the inverse, over the valid pairs only
    unspecified(layout, J, S, pitch)   bool per word of the extent: the positions the header leaves unspecified
                                       (rows J .. 16 * ceil(J / 16) - 1 of the tiles layout, nothing else)
    check_pitch(S, pitch, bit_planes)  the header's rule for the PE_MASK_ROWS pitch
"""
import numpy as np

NODE_TILES, JOB_BITS, NODE_BLOCKS, ROWS = 0, 1, 2, 3
LAYOUTS = (NODE_TILES, JOB_BITS, NODE_BLOCKS, ROWS)

JOB_BITS_NODE_ROUND = 1024      # "S rounded up to 1024"
LINE_WORDS = 16                 # a 128-byte line
BLOCK_WORDS = 128               # an 8192-node block of one row


def _ceil(a, b):
    return -(-a // b)


def words_per_row(S):
    return _ceil(S, 64)


def job_bits_stride(S):
    return _ceil(S, JOB_BITS_NODE_ROUND) * JOB_BITS_NODE_ROUND


def check_pitch(S, pitch, bit_planes):
    """The pitch of PE_MASK_ROWS as the header states it: at least words_per_row, a whole number of 128-byte
    lines, and on the bit-plane path a whole number of 8192-node blocks."""
    assert pitch >= words_per_row(S), (S, pitch)
    assert pitch % LINE_WORDS == 0, (S, pitch)
    if bit_planes:
        assert pitch % BLOCK_WORDS == 0, (S, pitch)


def extent(layout, J, S, pitch=0):
    Wn = words_per_row(S)
    if layout == NODE_TILES:
        return _ceil(J, 16) * _ceil(Wn, 4) * 64
    if layout == JOB_BITS:
        return _ceil(J, 64) * job_bits_stride(S)
    if layout == NODE_BLOCKS:
        return _ceil(S, 8192) * J * 128
    if layout == ROWS:
        assert pitch >= Wn, (pitch, Wn)
        return J * pitch
    raise ValueError(layout)


def word_index(layout, J, S, pitch=0):
    """int64 [J][Wn]: where word (j, c) sits -- for PE_MASK_JOB_BITS [ceil(J / 64)][S]: where word (b, n) sits."""
    Wn = words_per_row(S)
    if layout == JOB_BITS:
        b = np.arange(_ceil(J, 64), dtype=np.int64)[:, None]
        n = np.arange(S, dtype=np.int64)[None, :]
        return b * job_bits_stride(S) + n
    j = np.arange(J, dtype=np.int64)[:, None]
    c = np.arange(Wn, dtype=np.int64)[None, :]
    if layout == NODE_TILES:
        return ((j // 16) * _ceil(Wn, 4) + c // 4) * 64 + (j % 16) * 4 + c % 4
    if layout == NODE_BLOCKS:
        return ((c // 128) * J + j) * 128 + c % 128
    if layout == ROWS:
        return j * pitch + c
    raise ValueError(layout)


def _node_mask(S):
    """uint64 [Wn]: the bits of each row word that are nodes of the shard."""
    m = np.full(words_per_row(S), ~np.uint64(0), dtype=np.uint64)
    if S % 64:
        m[-1] = np.uint64((1 << (S % 64)) - 1)
    return m


def _to_job_bits(rows, J, S):
    """[J][Wn] node-bit rows -> [ceil(J / 64)][S] job-bit words."""
    bits = np.unpackbits(np.ascontiguousarray(rows, dtype="<u8").view(np.uint8), axis=1, bitorder="little")[:, :S]
    B = _ceil(J, 64)
    padded = np.zeros((B * 64, S), dtype=np.uint8)
    padded[:J] = bits
    per_band = padded.reshape(B, 64, S).transpose(0, 2, 1)            # [B][S][64]: bit j % 64 of word (b, n)
    return np.ascontiguousarray(np.packbits(per_band, axis=2, bitorder="little")).view("<u8").reshape(B, S)


def _from_job_bits(words, J, S):
    B = _ceil(J, 64)
    per_band = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8).reshape(B, S, 8), axis=2,
                             bitorder="little")                       # [B][S][64]
    bits = per_band.transpose(0, 2, 1).reshape(B * 64, S)[:J]
    Wn = words_per_row(S)
    padded = np.zeros((J, Wn * 64), dtype=np.uint8)
    padded[:, :S] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(J, Wn)


def image(rows, layout, J, S, pitch=0):
    rows = np.asarray(rows, dtype=np.uint64)
    assert rows.shape == (J, words_per_row(S)), (rows.shape, J, S)
    img = np.zeros(extent(layout, J, S, pitch), dtype=np.uint64)
    idx = word_index(layout, J, S, pitch)
    if layout == JOB_BITS:
        img[idx.reshape(-1)] = _to_job_bits(rows, J, S).reshape(-1)
    else:
        img[idx.reshape(-1)] = (rows & _node_mask(S)[None, :]).reshape(-1)
    return img


def rows_of(img, layout, J, S, pitch=0):
    img = np.asarray(img, dtype=np.uint64)
    assert img.shape == (extent(layout, J, S, pitch),), (img.shape, layout, J, S, pitch)
    idx = word_index(layout, J, S, pitch)
    if layout == JOB_BITS:
        return _from_job_bits(img[idx], J, S)
    return img[idx] & _node_mask(S)[None, :]


def unspecified(layout, J, S, pitch=0):
    out = np.zeros(extent(layout, J, S, pitch), dtype=bool)
    if layout == NODE_TILES and J % 16:
        Wt = _ceil(words_per_row(S), 4)
        j = np.arange(J, _ceil(J, 16) * 16, dtype=np.int64)[:, None]
        c = np.arange(4 * Wt, dtype=np.int64)[None, :]
        out[(((j // 16) * Wt + c // 4) * 64 + (j % 16) * 4 + c % 4).reshape(-1)] = True
    return out
