"""The select sweep's 16x16x32 tile (k_logits_f16x<.., kOutUB, .., kMfma16>, csrc/score.hip) on a machine without a GPU: its lane and
register arithmetic lives in csrc/sweep_layout.h, which libsixdgs_hostcheck.so instantiates for the host.  Over the 64 lanes of a wave every
(register, lane) is walked through

    accumulator (token block, ray block, register) -> (token, ray)   ->   sum of the lane's 4 token blocks   ->   halving butterfly over the
    16 token lanes   ->   the two stores per lane

with SETS of (token, ray) standing in for the values: the accumulators must cover the wave's 64 tokens x 128 rays exactly once, every one of
the 128 rays must be written exactly once and hold all 64 tokens of that ray and nothing else, the ragged mask must zero exactly the rays
beyond the tile's last one, and the per-token merge must put every token's four lane groups into the four rows of the merge buffer."""
import ctypes as C
import importlib

import pytest


@pytest.fixture(scope="module")
def hc():
    b = importlib.import_module("6dgs_amd.build")
    lib = C.CDLL(b.build_hostcheck())
    lib.hc_sw_frag_offset.restype = C.c_uint
    return lib


LANES = range(64)


def test_constants(hc):
    assert [hc.hc_sw_const(i) for i in range(4)] == [4, 8, 2048, 4]


def test_accumulators_cover_the_wave_tile_once(hc):
    seen = {}
    for lane in LANES:
        for tb in range(4):
            for rb in range(8):
                for reg in range(4):
                    key = (hc.hc_sw_acc_token(lane, tb), hc.hc_sw_acc_ray(lane, rb, reg))
                    assert key not in seen, (key, seen[key], (lane, tb, rb, reg))
                    seen[key] = (lane, tb, rb, reg)
        # the 16x16 C/D map itself: column = lane & 15, row = 4 (lane >> 4) + register
        assert hc.hc_sw_acc_token(lane, 0) == lane & 15 and hc.hc_sw_acc_ray(lane, 0, 0) == 4 * (lane >> 4)
    assert set(seen) == {(t, r) for t in range(64) for r in range(128)}


def _butterfly(hc, masked=lambda ray: False):
    """-> out[lane][x] = set of (token, ray) summed into the lane's output x (masked rays contribute nothing)."""
    v = []
    for lane in LANES:
        row = []
        for i in range(32):
            rb, reg = i >> 2, i & 3
            s = set()
            for tb in range(4):                                   # the lane's 4 token blocks add up in registers
                ray = hc.hc_sw_acc_ray(lane, rb, reg)
                if not masked(ray):
                    s.add((hc.hc_sw_acc_token(lane, tb), ray))
            row.append({i: s})
        v.append({i: row[i][i] for i in range(32)})
    for step in range(hc.hc_sw_const(3)):
        nxt = []
        for lane in LANES:
            p = hc.hc_sw_bfly_partner(lane, step)
            assert p != lane and p >> 4 == lane >> 4 and hc.hc_sw_bfly_partner(p, step) == lane     # pairs inside the 16 token lanes
            mine = {}
            for i, s in v[lane].items():
                if hc.hc_sw_bfly_keeps(lane, step, i):
                    j = i ^ (1 << step)
                    assert j in v[lane] and not hc.hc_sw_bfly_keeps(lane, step, j)              # of every pair one stays, one leaves
                    assert i in v[p] and not hc.hc_sw_bfly_keeps(p, step, i)                   # and the partner sends the one that stays here
                    mine[i] = s | v[p][i]
            assert 2 * len(mine) == len(v[lane])
            nxt.append(mine)
        v = nxt
    out = []
    for lane in LANES:
        assert sorted(v[lane]) == sorted(hc.hc_sw_out_index(lane, x) for x in range(2))
        out.append([v[lane][hc.hc_sw_out_index(lane, x)] for x in range(2)])
    return out


def test_butterfly_and_stores_write_every_ray_once(hc):
    out = _butterfly(hc)
    written = {}
    for lane in LANES:
        for x in range(2):
            ray = hc.hc_sw_out_ray(lane, x)
            assert ray not in written, (ray, written[ray], lane)
            written[ray] = lane
            assert out[lane][x] == {(t, ray) for t in range(64)}, (lane, x)               # all 4 token blocks of all 16 token lanes, this ray only
    assert sorted(written) == list(range(128))
    for x in range(2):                                                                       # one store instruction: 64 consecutive rays
        assert sorted(hc.hc_sw_out_ray(lane, x) for lane in LANES) == list(range(64 * x, 64 * x + 64))


@pytest.mark.parametrize("lim_cur", [0, 1, 15, 16, 17, 127, 128, 254])
def test_ragged_tile_zeroes_exactly_the_rays_beyond_the_last(hc, lim_cur):
    """lim_cur = index of the tile's last valid ray (of 256); the kernel masks accumulator (lane, rb, reg) of wave column wn when
    128 wn + acc_ray > lim_cur."""
    for wn in range(2):
        out = _butterfly(hc, masked=lambda ray: 128 * wn + ray > lim_cur)
        for lane in LANES:
            for x in range(2):
                ray = hc.hc_sw_out_ray(lane, x)
                want = {(t, ray) for t in range(64)} if 128 * wn + ray <= lim_cur else set()
                assert out[lane][x] == want, (wn, lane, x)


def test_token_merge_fills_the_four_rows(hc):
    """g_t: per token the 4 lane groups lane >> 4 of either wave column hold partial sums; lanes with part_writes take the partner lane ^ 16."""
    rows = {}
    for wn in range(2):
        for lane in LANES:
            if not hc.hc_sw_part_writes(lane):
                assert hc.hc_sw_part_writes(lane ^ 16)
                continue
            for tb in range(4):
                assert hc.hc_sw_acc_token(lane ^ 16, tb) == hc.hc_sw_acc_token(lane, tb)
                key = (hc.hc_sw_part_row(wn, lane), hc.hc_sw_acc_token(lane, tb))
                assert key not in rows
                rows[key] = {(wn, lane >> 4), (wn, (lane ^ 16) >> 4)}
    assert set(rows) == {(h, t) for h in range(4) for t in range(64)}
    for t in range(64):
        groups = set().union(*(rows[(h, t)] for h in range(4)))
        assert groups == {(wn, g) for wn in range(2) for g in range(4)}


def test_fragment_reads_are_conflict_free_on_the_swizzled_image(hc):
    """ds_read_b128 is served in four groups of 16 lanes; within a group the 16-byte reads must fall on 16 distinct bank groups
    ((address / 16) mod 16).  Lane l reads row l & 15 of its block, chunk plane * 4 + (l >> 4), XOR-swizzled with (row >> 1) & 7."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in g] for g in groups]
    for row0 in range(0, 256, 16):
        for plane in range(2):
            for lane in LANES:
                off = hc.hc_sw_frag_offset(row0, lane, plane)
                row = row0 + hc.hc_sw_frag_row(lane)
                assert off // 128 == row and ((off % 128) // 16) ^ ((row >> 1) & 7) == hc.hc_sw_frag_chunk(lane, plane)
                assert hc.hc_sw_frag_chunk(lane, plane) == plane * 4 + (lane >> 4)
            for g in groups:
                banks = {(hc.hc_sw_frag_offset(row0, lane, plane) // 16) % 16 for lane in g}
                assert len(banks) == 16, (row0, plane, g)
