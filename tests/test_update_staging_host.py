"""Host restatement of the row schedules of dwxh_kernel and dx1w1_kernel2 (csrc/tsc_model.hip): which sub-chunks / chunks of a
split run unclamped, what the LDS ring of dwxh holds when it is read, and which rows an unclamped load may touch.  No GPU: the
model walks the same loop conditions and asserts, for every split length,
  * each 16-row sub-chunk's MFMAs read the ring slot that holds exactly its rows, and its dZ operands are its own;
  * no slot is written between the two barriers around a read of it (either order of staging and MFMAs inside a sub-chunk,
    any drift between wavefronts inside an interval);
  * every unclamped load lies inside the split, and a sub-chunk whose MFMAs run unclamped has no row past the split;
  * every sub-chunk is used exactly once, in ascending order (the accumulation order of the kernel before the ring).
It also pins what the shapes of tests/test_update_staging_gpu.py drive (the counts quoted in its docstring)."""
KC, S_UPD = 16, 5


def dwxh_schedule(R):
    """-> (sub-chunks in the order their MFMAs run, unclamped intervals, clamped sub-chunks, barriers in the loops)"""
    ring, written, read = [None] * 8, set(), set()
    used, plain, clamped, barriers = [], 0, 0, 0
    if R <= 0:
        return used, plain, clamped, barriers

    def load(clamp, c):                       # rows [KC c, KC c + KC) of the split
        assert clamp or KC * (c + 1) <= R, ('unclamped load past the split', R, c)
        return c

    for c in range(4):
        ring[c] = load(True, c)
    regs, bcur = load(True, 4), load(True, 0)

    def sub(clamp, c):
        nonlocal regs, bcur
        assert clamp or KC * (c + 1) <= R, ('unclamped MFMA rows past the split', R, c)
        bnxt = load(clamp, c + 1)
        slot = (c + 4) & 7                    # commit_a(c + 4): before or after the MFMAs, so it must not meet any read
        assert regs == c + 4
        ring[slot] = regs
        written.add(slot)
        regs = load(clamp, c + 5)
        assert ring[c & 7] == c and bcur == c
        read.add(c & 7)
        assert not (written & read), ('slot written and read between two barriers', R, c)
        used.append(c)
        bcur = bnxt

    c = 0
    while KC * (c + 9) <= R:
        for j in range(4):
            sub(False, c + j)
        written.clear(); read.clear(); barriers += 1
        plain += 1
        c += 4
    while KC * c < R:
        sub(True, c)
        clamped += 1
        if c & 3 == 3:
            written.clear(); read.clear(); barriers += 1
        c += 1
    return used, plain, clamped, barriers


def dx1w1_schedule(R):
    """-> (unclamped chunks, clamped chunks) of a split of R rows"""
    plain = clamped = 0
    row = 0
    while row + 64 <= R:                      # the chunk's rows and the successor it requests lie inside the split
        plain += 1
        row += 32
    while row < R:
        clamped += 1
        row += 32
    assert 32 * (plain + clamped) >= R > 32 * (plain + clamped - 1) or R <= 0
    return plain, clamped


def splits(N, mult):
    rps = -(-N // S_UPD)
    rps = -(-rps // mult) * mult
    return rps, [max(0, min(N, (s + 1) * rps) - s * rps) for s in range(S_UPD)]


def test_dwxh_schedule_is_sound():
    for R in list(range(0, 700)) + [3840, 4096, 24576, 24577, 24590]:
        used, plain, clamped, barriers = dwxh_schedule(R)
        assert used == list(range(-(-max(R, 0) // KC))), R
        assert 4 * plain + clamped == len(used), R
        assert plain == max(0, (R // KC - 5) // 4), R


def test_dx1w1_schedule_covers_the_split():
    for R in list(range(0, 400)) + [24576]:
        plain, clamped = dx1w1_schedule(R)
        assert plain + clamped == -(-R // 32), R
        assert clamped == min(-(-R // 32), 2 if R % 32 else 1), R


def test_shapes_of_the_gpu_test_drive_every_path():
    # E * T of tests/test_update_staging_gpu.py on large_grid (50 towers -> 5 splits)
    want = {                                  # N: (dwxh rps, [(R, intervals, clamped sub-chunks)], dx1w1 rps, [(R, plain, clamped)])
        1: (2, [(1, 0, 1)] + [(0, 0, 0)] * 4, 32, [(1, 0, 1)] + [(0, 0, 0)] * 4),
        21: (6, [(6, 0, 1)] * 3 + [(3, 0, 1), (0, 0, 0)], 32, [(21, 0, 1)] + [(0, 0, 0)] * 4),
        429: (86, [(86, 0, 6)] * 4 + [(85, 0, 6)], 96, [(96, 2, 1)] * 4 + [(45, 0, 2)]),
        825: (166, [(166, 1, 7)] * 4 + [(161, 1, 7)], 192, [(192, 5, 1)] * 4 + [(57, 0, 2)]),
        1280: (256, [(256, 2, 8)] * 5, 256, [(256, 7, 1)] * 5),
    }
    for N, (rps_w, dw, rps_x, dx) in want.items():
        r, sp = splits(N, 2)
        assert r == rps_w
        assert [(R,) + dwxh_schedule(R)[1:3] for R in sp] == dw, N
        r, sp = splits(N, 32)
        assert r == rps_x
        assert [(R,) + dx1w1_schedule(R) for R in sp] == dx, N
    # the ragged transition: unclamped intervals, then a clamped tail whose last sub-chunk is short, and an odd last split
    assert 166 % KC == 6 and 161 % 2 == 1 and 161 % KC == 1
