"""Host restatement of dwxh_split_kernel (csrc/tsc_model.hip): its LDS image, its row schedule and the three-way bf16 split.  No GPU.
  * Image.  A 16-row sub-chunk of [X1 | h_prev] lives in LDS as three bf16 planes (one per piece).  The staging threads write 8-byte
    groups of four features at dwxh_split_off; the MFMA fragments come back through ds_read_b64_tr_b16, modelled here as the ISA
    describes it (per 16-lane group a block of 4 rows x 16 elements, lane 4q + p supplies the address of row q, elements 4p .. 4p+3,
    lane i receives element i of the four rows).  Asserted for every width: the writes tile the planes exactly once (a bijection), every
    lane's fragment holds (piece, row 8h + j, feature 32t + r) for j = 0 .. 7, and a 32-lane half of a read touches 64 distinct banks.
  * Schedule.  Ring of four sub-chunks, a barrier every two: each sub-chunk's MFMAs read the slot that holds exactly its rows, no slot
    is written between the barriers around a read of it, unclamped loads stay inside the split, every row is consumed once.
  * Split.  p1 = bf16(x), p2 = bf16(x - p1), p3 = bf16((x - p1) - p2), round to nearest even: p1 + p2 + p3 == x exactly.
It also counts what the shapes of tests/test_dwxh_split_gpu.py drive.
What is NOT pinned here is which piece products reach the accumulator: tests/split_harness.py restates that (the six products, mutants
that lose or misplace one), tests/test_split_mutants_host.py holds the mutant table, and the exact probes of the GPU test pin it bit
for bit on the kernel."""
import numpy as np
import torch

KC, L = 16, 64
WIDTHS = (128, 160, 192, 224)


def off(NT, rr, f):
    """dwxh_split_off: byte offset of features f .. f + 3 of row rr inside a piece's plane"""
    return ((rr >> 3) * NT + (f >> 5)) * 512 + 64 * (rr & 7) + 16 * (((f >> 3) & 3) ^ ((rr >> 2) & 3)) + 2 * (f & 7)


def staging_slots(H, tid):
    """(row, first feature in [X1 | h_prev]) of every float4 thread tid stages per sub-chunk: dwxh_kernel's slots"""
    XQ = H // 4
    NX = KC * XQ
    wave = tid >> 6
    out = [(tid // XQ, 4 * (tid % XQ))]
    if wave < (NX - 512) // 64:
        i1 = tid + 512
        out.append((i1 // XQ, 4 * (i1 % XQ)))
    if wave >= 4:
        i2 = tid & 255
        out.append((i2 >> 4, H + 4 * (i2 & 15)))
    return out


def fill_image(H):
    """-> int32 image of one sub-chunk, one entry per bf16: piece << 24 | row << 16 | feature; asserts the writes are a bijection"""
    NT = (H + L) // 32
    PL = 2 * KC * NT * 32
    img = np.full(3 * PL // 2, -1, np.int64)
    for tid in range(512):
        for rr, f in staging_slots(H, tid):
            assert 0 <= rr < KC and f % 4 == 0 and f + 3 < H + L
            for piece in range(3):
                o = off(NT, rr, f) + piece * PL
                assert o % 8 == 0
                for e in range(4):
                    assert img[o // 2 + e] == -1, ('two writes to one slot', H, tid, rr, f)
                    img[o // 2 + e] = piece << 24 | rr << 16 | (f + e)
    assert (img >= 0).all(), ('slots never written', H)
    return img, NT, PL


def read_bases(NT, lane):
    kh, rq, rp = lane >> 5, (lane >> 2) & 3, lane & 3
    rc = 2 * ((lane >> 4) & 1) + (rp >> 1)
    rb0 = kh * NT * 512 + 64 * rq + 16 * (rc ^ (2 * kh)) + 8 * (rp & 1)
    rb1 = kh * NT * 512 + 64 * (4 + rq) + 16 * (rc ^ (2 * kh + 1)) + 8 * (rp & 1)
    return rb0, rb1


def tr_read(img, addr):
    """ds_read_b64_tr_b16 of one wave: addr[64] byte addresses -> [64][4] elements"""
    out = np.zeros((64, 4), np.int64)
    for lane in range(64):
        g, i = lane & ~15, lane & 15
        for q in range(4):
            a = addr[g + 4 * q + (i >> 2)]
            assert a % 8 == 0
            out[lane, q] = img[a // 2 + (i & 3)]
    return out


def test_image_is_a_bijection_and_fragments_match_the_operand_map():
    for H in WIDTHS:
        img, NT, PL = fill_image(H)
        assert 4 * 3 * PL <= 160 * 1024                      # the ring of four sub-chunks
        bases = [read_bases(NT, lane) for lane in range(64)]
        for t in range(NT):
            for piece in range(3):
                for s in range(2):
                    addr = [bases[lane][s] + piece * PL + t * 512 for lane in range(64)]
                    assert max(addr) + 8 <= 3 * PL
                    for half in (0, 32):                     # bank (a / 4) % 64 per 32-lane half, two dwords per lane
                        banks = {(a // 4 + d) % 64 for a in addr[half:half + 32] for d in (0, 1)}
                        assert len(banks) == 64, ('bank conflict', H, t, piece, s)
                    got = tr_read(img, addr)
                    for lane in range(64):
                        r, h = lane & 31, lane >> 5
                        for q in range(4):
                            assert got[lane, q] == (piece << 24 | (8 * h + 4 * s + q) << 16 | (32 * t + r)), (H, t, piece, s, lane, q)


def schedule(R):
    """-> (sub-chunks in the order their MFMAs run, unclamped intervals, clamped sub-chunks)"""
    ring, written, read = [None] * 4, set(), set()
    used, plain, clamped = [], 0, 0
    if R <= 0:
        return used, plain, clamped

    def load(clamp, c):
        assert clamp or KC * (c + 1) <= R, ('unclamped load past the split', R, c)
        return c

    for c in range(2):
        ring[c] = load(True, c)
    regs, bcur = load(True, 2), load(True, 0)

    def sub(clamp, c):
        nonlocal regs, bcur
        assert clamp or KC * (c + 1) <= R, ('unclamped MFMA rows past the split', R, c)
        bnxt = load(clamp, c + 1)
        slot = (c + 2) & 3                    # commit_a(c + 2): before or after the MFMAs, so it must not meet any read
        assert regs == c + 2
        ring[slot] = regs
        written.add(slot)
        regs = load(clamp, c + 3)
        assert ring[c & 3] == c and bcur == c
        read.add(c & 3)
        assert not (written & read), ('slot written and read between two barriers', R, c)
        used.append(c)
        bcur = bnxt

    c = 0
    while KC * (c + 5) <= R:
        sub(False, c); sub(False, c + 1)
        written.clear(); read.clear()
        plain += 1
        c += 2
    while KC * c < R:
        sub(True, c)
        clamped += 1
        if c & 1:
            written.clear(); read.clear()
        c += 1
    return used, plain, clamped


def test_schedule_is_sound():
    for R in list(range(0, 700)) + [24576]:
        used, plain, clamped = schedule(R)
        assert used == list(range(-(-R // KC))), R
        assert 2 * plain + clamped == len(used), R
        assert plain == max(0, (R // KC - 3) // 2), R


def splits(N, S):
    rps = -(-N // S)
    rps = -(-rps // 2) * 2
    return [max(0, min(N, (s + 1) * rps) - s * rps) for s in range(S)]


# N of tests/test_dwxh_split_gpu.py with S = 5 -> [(R, unclamped intervals, clamped sub-chunks)]
GPU_SHAPES = {
    1: [(1, 0, 1)] + [(0, 0, 0)] * 4,                         # one row, four empty splits
    21: [(6, 0, 1)] * 3 + [(3, 0, 1), (0, 0, 0)],             # splits shorter than one 16-row step, an empty one
    349: [(70, 0, 5)] * 4 + [(69, 0, 5)],                     # odd last split, no unclamped interval (R < 80), across two barriers
    409: [(82, 1, 4)] * 4 + [(81, 1, 4)],                     # last split: one unclamped interval, then a single-row last step
    1280: [(256, 6, 4)] * 5,                                  # every row valid
}


def test_shapes_of_the_gpu_test_drive_every_path():
    for N, want in GPU_SHAPES.items():
        assert [(R,) + schedule(R)[1:] for R in splits(N, 5)] == want, (N, [(R,) + schedule(R)[1:] for R in splits(N, 5)])
    assert 69 % 2 == 1 and 81 % KC == 1 and 81 >= 5 * KC


def split3(x):
    p1 = x.to(torch.bfloat16)
    r1 = x - p1.float()
    p2 = r1.to(torch.bfloat16)
    p3 = (r1 - p2.float()).to(torch.bfloat16)
    return p1, p2, p3


def test_three_way_split_reconstructs_f32_exactly():
    rng = np.random.RandomState(0)
    full = (rng.randint(1 << 23, 1 << 24, 20000).astype(np.float64) * 2.0 ** rng.randint(-30, 30, 20000)).astype(np.float32)    # 24-bit mantissas
    full[::2] *= -1
    assert ((np.abs(full).view(np.uint32) & 1) == 1).sum() > 5000               # lowest mantissa bit set: nothing to spare
    ties = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -9, -(1 + 2.0 ** -8), -(1 + 2.0 ** -9), 1 + 2.0 ** -8 + 2.0 ** -16, 1 + 2.0 ** -9 + 2.0 ** -17,
                     1 + 3 * 2.0 ** -9, 1 - 2.0 ** -9, 1 - 2.0 ** -10], np.float32)
    wide = (rng.uniform(1, 2, 20000) * 2.0 ** rng.uniform(-100, 100, 20000) * rng.choice([-1, 1], 20000)).astype(np.float32)
    ones = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -100, 2.0 ** 100, np.float32(np.nextafter(np.float32(2), np.float32(0)))], np.float32)
    for v in (full, ties, wide, ones):
        x = torch.from_numpy(v.copy())
        p1, p2, p3 = split3(x)
        back = (p1.double() + p2.double() + p3.double()).numpy()
        assert np.array_equal(back, v.astype(np.float64)), v[back != v.astype(np.float64)][:5]
        # and the sum as the kernel's accumulators see it: f32, smallest first
        assert np.array_equal(((p3.float() + p2.float()) + p1.float()).numpy(), v)
