"""The block-wise epilogue of the select sweep's 16x16x32 tile (csrc/score.hip: SweepEpi, k_logits_f16x<kAllTerms, kOutUB, PERS, kMfma16>) lives on
the registers the per-tile form left free -- a spill inside the tile costs more than the overlap gives (the first 16x16x32 build lost all its
gain to 34 spilled registers).  From the cross-compile, for the persistent and the one-shot grid:

  * 1152 MFMAs and 288 ds_read_b128 in the tile (the pieces add neither matrix work nor fragment reads; the drain behind the tile loop has none);
  * 32 of those MFMAs take the inline constant 0 as C -- slab 0 starts every accumulator from it, there is no zeroing sweep and no second set;
  * all 128 v_exp_f32 of a tile's epilogue sit between the tile's MFMAs (the drain has its own 64);
  * no scratch access inside the tile;
  * spilled VGPRs and scratch bytes per lane not above the per-tile form's before this change (persistent 6 / 28 B, one-shot 0 / 0);

the per-tile form is still there behind SIXDGS_SWEEP_EPILOGUE=tile (SHAPE 2: 1152 MFMAs, no v_exp_f32 between them), and every 32x32x16 instance compiles to
the code it compiled to before: the hashes below are those of `tools/kernel_resources.py --digest` (instruction stream without comments and
block-label numbers) on the commit before the block-wise epilogue, same compiler.  A compiler update moves all of them at once; regenerate them
then from that commit."""
import hashlib
import importlib
import os
import re
import subprocess
import tempfile

import pytest

# <TERMS, OUT, PERS, SHAPE 0 (kMfma32)> -> code hash: the two-pass outputs, the four pre-pass instances, the two behind SIXDGS_SWEEP_MFMA=32
PARENT_32X32X16 = {
    "ILi3ELi1ELb0ELi0EE": "d477c30a9b264bb0",
    "ILi3ELi0ELb0ELi0EE": "e6350ae3aff0446e",
    "ILi1ELi2ELb1ELi0EE": "4ded0a01f0860c6e",
    "ILi3ELi2ELb1ELi0EE": "6bb6ea80c1bf646e",
    "ILi1ELi2ELb0ELi0EE": "01cd5c552d7d5a3d",
    "ILi3ELi2ELb0ELi0EE": "885431fd9b069919",
    "ILi3ELi3ELb1ELi0EE": "bbdac64849e024ec",
    "ILi3ELi3ELb0ELi0EE": "66795ab7e8666839",
}


@pytest.fixture(scope="module")
def compiled():
    b = importlib.import_module("6dgs_amd.build")
    src = os.path.join(b.CSRC, "score.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "score.s")
        subprocess.run([b.HIPCC, *[f for f in b.FLAGS if not f.startswith("-DSDG_")], "--cuda-device-only", "-S", src, "-o", asm], capture_output=True, text=True, check=True)
        text = open(asm).read()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        blk = m.group(0)
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = (g("vgpr_spill_count"), g("private_segment_fixed_size"))
    return meta, text


def body_of(text, name):
    body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\s*\.section\s+\.rodata", text, re.S | re.M).group(1)
    return [l.split(";")[0].strip() for l in body.splitlines() if l.split(";")[0].strip()]


def code_hash(text, name):
    body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\s*\.section\s+\.rodata", text, re.S | re.M).group(1)
    body = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";[^\n]*", "", body))
    return hashlib.sha256("\n".join(ln.strip() for ln in body.splitlines() if ln.strip()).encode()).hexdigest()[:16]


def one(meta, tag):
    names = [k for k in meta if "k_logits_f16x" + tag in k]
    assert len(names) == 1, (tag, sorted(meta))
    return names[0]


def tile_of(body):
    """From the tile's first MFMA to the first branch behind its last one (the last slab's last fragment read sits behind the last MFMA)."""
    mfma = [i for i, l in enumerate(body) if l.startswith("v_mfma_f32_16x16x32_f16")]
    end = next(i for i in range(mfma[-1], len(body)) if body[i].startswith(("s_cbranch", "s_branch")))
    return mfma, body[mfma[0]:end]


@pytest.mark.parametrize("pers,max_spilled,max_scratch", [(1, 6, 28), (0, 0, 0)])
def test_block_wise_epilogue_fits_the_tile(compiled, pers, max_spilled, max_scratch):
    meta, text = compiled
    name = one(meta, f"ILi3ELi3ELb{pers}ELi1EE")
    spilled, scratch = meta[name]
    body = body_of(text, name)
    mfma, tile = tile_of(body)
    reads = sum(l.startswith("ds_read_b128") for l in tile)
    zero_c = sum(bool(re.search(r",\s*0$", body[i])) for i in mfma)
    exps_tile, exps_all = sum(l.startswith("v_exp_f32") for l in tile), sum(l.startswith("v_exp_f32") for l in body)
    print(f"[sweep epilogue resources] PERS={pers}: {len(mfma)} MFMAs ({zero_c} from C = 0), {reads} ds_read_b128, v_exp_f32 {exps_tile} in the tile of {exps_all}, "
          f"{spilled} spilled VGPRs, scratch {scratch} B/lane")
    assert len(mfma) == 1152, len(mfma)
    assert reads == 288, reads
    assert zero_c == 32, zero_c
    assert exps_tile == 128 and exps_all == 128 + 64 + 8, (exps_tile, exps_all)      # (+ 8: the merge of the token partials behind the group)
    inside = [l for l in tile if "scratch_" in l]
    assert not inside, inside[:3]
    assert spilled <= max_spilled, spilled
    assert scratch <= max_scratch, scratch


@pytest.mark.parametrize("pers", [1, 0])
def test_per_tile_epilogue_stays_behind_the_switch(compiled, pers):
    meta, text = compiled
    body = body_of(text, one(meta, f"ILi3ELi3ELb{pers}ELi2EE"))
    mfma, _ = tile_of(body)
    between = body[mfma[0]:mfma[-1]]
    assert len(mfma) == 1152, len(mfma)
    assert not any(l.startswith("v_exp_f32") for l in between)      # the whole epilogue behind the last MFMA
    assert not [l for l in between if "scratch_" in l]


@pytest.mark.parametrize("tag", sorted(PARENT_32X32X16))
def test_32x32x16_instances_compile_to_the_same_code(compiled, tag):
    meta, text = compiled
    assert code_hash(text, one(meta, tag)) == PARENT_32X32X16[tag]
