"""Host restatement of dx1w1_split_kernel (csrc/tsc_model.hip): the truncating three-way cut of the stationary weights, the LDS image of a
dZ chunk with the permuted contraction index, and the chunk loop.  No GPU.
  * Cut.  p1 = x & 0xffff0000, p2 = (x - p1) & 0xffff0000, p3 = ((x - p1) - p2) & 0xffff0000, with the kernel's integer and f32
    operations (the byte permute that packs two pieces keeps their high halves).  p1 + p2 + p3 == x exactly for every x that three
    bf16 can hold at all: every multiple of 2^-133, bf16's smallest subnormal, which covers every normal from 2^-110 up, every power of
    two and the subnormals down to 2^-133.  Below that no method is exact (a value with bits under 2^-133 is not a sum of bf16s): the
    cut then drops only those bits, |x - (p1 + p2 + p3)| < 2^-133, and never touches the bits from 2^-133 up.
  * Image.  A 32-row chunk of dZ lives in LDS as three planes [row tile 2][K-step 8][kq 4][row 16][8 bf16].  Asserted: the staging writes
    tile a plane exactly once; the fragment lane (n, kq) reads with ONE 16-byte read at 16 lane + a constant holds, in element order,
    exactly the k of the weight registers bw[8 s + e] = Wx^T[16 (2 s + (e >> 2)) + 4 kq + (e & 3)] that form its B fragment; each of
    the four 16-lane groups of a ds_read_b128 touches 64 distinct banks, and a wave's ds_write_b64 puts four lanes on every bank.
  * Loop.  Chunks of 32 rows, unclamped while the successor is whole; it also counts what the shapes of tests/test_dx1w1_split_gpu.py drive.
What is NOT pinned here is which piece products reach the accumulator: tests/split_harness.py restates that (this cut for Wx, the
rounding cut for dZ, the six products, mutants that lose or misplace one), tests/test_split_mutants_host.py holds the mutant table, and
the exact probes of the GPU test pin it bit for bit on the kernel."""
import numpy as np

PL = 2 * 8 * 4 * 16 * 16
HI = np.uint32(0xffff0000)


def cut3(x):
    """dx_cut8 on a float32 array -> three float32 arrays whose low halves are zero"""
    u = x.view(np.uint32)
    p1 = (u & HI).view(np.float32)
    r1 = x - p1
    p2 = (r1.view(np.uint32) & HI).view(np.float32)
    r2 = r1 - p2
    p3 = (r2.view(np.uint32) & HI).view(np.float32)
    return p1, p2, p3


def test_truncating_cut_reconstructs_f32_exactly():
    rng = np.random.RandomState(0)
    bits = rng.randint(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    bits = bits[((bits >> 23) & 0xff) != 0xff]                                  # finite values; subnormals stay in
    tiny = np.float32(2.0 ** -126)
    edges = np.array([0.0, -0.0, tiny, -tiny, np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.0, -1.0, 2.0 ** 100, 2.0 ** -100],
                     np.float32)
    low = (np.uint32(0x3f800000) | np.arange(1, 1 << 16, 257, dtype=np.uint32)).view(np.float32)          # only low mantissa bits set
    low1 = (np.uint32(0x3f800000) | (np.uint32(1) << np.arange(23, dtype=np.uint32))).view(np.float32)     # one mantissa bit each
    pow2 = (2.0 ** np.arange(-126, 128)).astype(np.float32)
    sub = np.concatenate([np.arange(1, 4096, dtype=np.uint32), np.uint32(0x007fffff) - np.arange(4096, dtype=np.uint32),
                          (np.uint32(1) << np.arange(23, dtype=np.uint32))]).view(np.float32)              # subnormals
    assert (np.abs(sub) < tiny).all() and (sub != 0).all()
    full = (bits | np.uint32(1)).view(np.float32)                                                          # lowest bit set: nothing to spare
    q = 2.0 ** -133                                                             # bf16's smallest subnormal
    seen_held = seen_low = 0
    for v in (bits.view(np.float32), full, edges, low, low1, pow2, sub, -sub):
        v = np.ascontiguousarray(v, np.float32)
        with np.errstate(all='raise'):
            p1, p2, p3 = cut3(v)
        for p in (p1, p2, p3):
            assert ((p.view(np.uint32) & np.uint32(0xffff)) == 0).all()         # each piece is a bf16
        v64 = v.astype(np.float64)
        back = p1.astype(np.float64) + p2.astype(np.float64) + p3.astype(np.float64)
        held = np.floor(v64 / q) * q == v64                                     # a multiple of 2^-133: three bf16 can hold it
        assert (held | (np.abs(v64) < 2.0 ** -110)).all()
        assert np.array_equal(back[held], v64[held])
        assert np.array_equal(((p3 + p2) + p1)[held], v[held])                  # as the f32 accumulator adds them, smallest first
        assert (np.abs(v64 - back)[~held] < q).all() and (np.abs(back) <= np.abs(v64)).all()
        assert np.array_equal(back[~held], np.trunc(v64[~held] / q) * q)        # only the bits below 2^-133 go
        assert (np.abs(p2) <= np.abs(p1) * 2.0 ** -7).all() and (np.abs(p3) <= np.abs(v) * 2.0 ** -15).all()
        seen_held += int(held.sum()); seen_low += int((~held).sum())
    assert seen_held > 190000 and seen_low > 1000


def staging(tid):
    """-> [(chunk row, first k, byte offset inside a plane)] of the four float4s thread tid stages"""
    wave, lane = tid >> 6, tid & 63
    zrow, zc0 = 8 * (wave & 3) + (lane >> 3), (lane & 7) + 8 * (wave >> 2)
    zl = (zrow >> 4) * 8192 + (wave >> 2) * 1024 + (lane & 3) * 256 + (zrow & 15) * 16 + ((lane >> 2) & 1) * 8
    return [(zrow, 4 * (zc0 + 16 * q), zl + 2048 * q) for q in range(4)]


def test_image_is_a_bijection_and_fragments_match_the_weight_registers():
    img = np.full(PL // 2, -1, np.int64)                       # one entry per bf16: row << 16 | k
    for tid in range(512):
        for row, k, o in staging(tid):
            assert 0 <= row < 32 and k % 4 == 0 and k + 3 < 256 and o % 8 == 0 and o + 8 <= PL
            for e in range(4):
                assert img[o // 2 + e] == -1, ('two writes to one slot', tid, row, k)
                img[o // 2 + e] = row << 16 | (k + e)
    assert (img >= 0).all()
    assert 2 * 3 * PL + 4 * 2 * 32 * 68 <= 160 * 1024          # two buffers of three planes + the obs chunks
    for r in range(2):
        for s in range(8):
            addr = [16 * lane + r * 8192 + s * 1024 for lane in range(64)]
            for lane in range(64):
                n, kq = lane & 15, lane >> 4
                for e in range(8):
                    k = 16 * (2 * s + (e >> 2)) + 4 * kq + (e & 3)                  # bw[8 s + e]
                    assert img[addr[lane] // 2 + e] == (16 * r + n) << 16 | k, (r, s, lane, e)
            # ds_read_b128: four 16-lane groups, bank (a / 4) % 64, four dwords per lane
            for grp in ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27), (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31)):
                for half in (0, 32):
                    banks = {(addr[half + l] // 4 + d) % 64 for l in grp for d in range(4)}
                    assert len(banks) == 64, ('bank conflict', r, s, grp)
    # ds_write_b64 of one wave: bank (a / 4) % 32, two dwords per lane; 512 bytes cannot take fewer than four lanes per bank
    for wave in range(8):
        for q in range(4):
            cnt = np.zeros(32, int)
            for lane in range(64):
                o = staging(64 * wave + lane)[q][2]
                cnt[(o // 4) % 32] += 1
                cnt[(o // 4 + 1) % 32] += 1
            assert (cnt == 4).all(), (wave, q, cnt)
    # global side: eight lanes read one aligned 128-byte line of a row
    for wave in range(8):
        for q in range(4):
            for l0 in range(0, 64, 8):
                rows = {staging(64 * wave + l)[q][0] for l in range(l0, l0 + 8)}
                ks = sorted(staging(64 * wave + l)[q][1] for l in range(l0, l0 + 8))
                assert len(rows) == 1 and ks == list(range(ks[0], ks[0] + 32, 4)) and ks[0] % 32 == 0


def chunks(R):
    """-> (plain chunks, clamped chunks, rows of the last chunk) of a split of R rows"""
    plain = clamped = 0
    row = 0
    if R <= 0:
        return 0, 0, 0
    while row + 64 <= R:
        plain += 1; row += 32
    last = 0
    while row < R:
        clamped += 1; last = min(32, R - row); row += 32
    return plain, clamped, last


def splits(N, S):
    rps = -(-(-(-N // S)) // 32) * 32
    return [max(0, min(N, (s + 1) * rps) - s * rps) for s in range(S)]


def test_chunk_loop_consumes_every_row_once():
    for R in list(range(0, 700)) + [24576]:
        plain, clamped, last = chunks(R)
        assert plain + clamped == -(-R // 32)
        assert plain == max(0, R // 32 - 1)                    # the last whole chunk runs clamped too: its successor is not whole
        if R:
            assert 32 * (plain + clamped - 1) + last == R


# N of tests/test_dx1w1_split_gpu.py with S = 5 -> [(R, plain chunks, clamped chunks, rows of the last chunk)]
GPU_SHAPES = {
    1: [(1, 0, 1, 1)] + [(0, 0, 0, 0)] * 4,
    21: [(21, 0, 1, 21)] + [(0, 0, 0, 0)] * 4,
    160: [(32, 0, 1, 32)] * 5,                                 # the plain loop is never entered
    161: [(64, 1, 1, 32)] * 2 + [(33, 0, 2, 1), (0, 0, 0, 0), (0, 0, 0, 0)],
    349: [(96, 2, 1, 32)] * 3 + [(61, 0, 2, 29), (0, 0, 0, 0)],               # the clamped tail ends inside row tile 1
    1280: [(256, 7, 1, 32)] * 5,
}


def test_shapes_of_the_gpu_test_drive_every_path():
    for N, want in GPU_SHAPES.items():
        got = [(R,) + chunks(R) for R in splits(N, 5)]
        assert got == want, (N, got)
        assert sum(R for R, *_ in got) == N
