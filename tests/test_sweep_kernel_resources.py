"""The select sweep's 16x16x32 instances (k_logits_f16x<kAllTerms, kOutUB, PERS, kMfma16>, csrc/score.hip) sit on the 256-register line like the
32x32x16 ones they replace: 128 accumulator registers, 44 fragment registers, and hipcc parks whatever no longer fits in scratch.  The resource
report and the assembly of the cross-compile must show, for the persistent and the one-shot grid:

  * 1152 v_mfma_f32_16x16x32_f16 (12 slabs x 8 ray blocks x 4 token blocks x 3 terms, one copy of the tile) and no 32x32x16 MFMA;
  * no scratch access between the first and the last MFMA of the tile;
  * scratch bytes per lane not above the 32x32x16 instances' (28 persistent, 8 one-shot: loop invariants of the group loop);
  * 163840 B of LDS (the rings are unchanged);

and the 32x32x16 instances of the sweep are still there behind the developer switch (576 MFMAs each)."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest


@pytest.fixture(scope="module")
def compiled():
    b = importlib.import_module("6dgs_amd.build")
    src = os.path.join(b.CSRC, "score.hip")
    with tempfile.TemporaryDirectory() as tmp:
        base = [b.HIPCC, *[f for f in b.FLAGS if not f.startswith("-DSDG_")], "--cuda-device-only"]
        asm = os.path.join(tmp, "score.s")
        rep = subprocess.run(base + ["-S", src, "-o", asm, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True).stderr
        text = open(asm).read()
    res = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rep, re.S):
        res[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return res, text


def body_of(text, name):
    body = text[text.index("\n" + name + ":"):]
    return [l.split(";")[0].strip() for l in body[:body.index("s_endpgm")].splitlines()]


# mangled template arguments: <TERMS 3, OUT 3 (kOutUB), PERS, SHAPE 1 (kMfma16)>
@pytest.mark.parametrize("pers,max_scratch", [(1, 28), (0, 8)])
def test_sweep_16x16x32_instances(compiled, pers, max_scratch):
    res, text = compiled
    names = [k for k in res if f"k_logits_f16xILi3ELi3ELb{pers}ELi1EE" in k]
    assert len(names) == 1, sorted(res)
    scratch, lds = res[names[0]]
    body = body_of(text, names[0])
    mfma = [i for i, l in enumerate(body) if l.startswith("v_mfma_f32_16x16x32_f16")]
    print(f"[sweep resources] PERS={pers}: {len(mfma)} MFMAs, scratch {scratch} B/lane, LDS {lds} B")
    assert len(mfma) == 1152, len(mfma)
    assert not [l for l in body if "v_mfma_f32_32x32x16_f16" in l]
    inside = [l for l in body[mfma[0]:mfma[-1]] if "scratch_" in l]
    assert not inside, inside[:3]
    assert scratch <= max_scratch, scratch
    assert lds == 163840, lds


@pytest.mark.parametrize("pers", [1, 0])
def test_sweep_32x32x16_instances_stay_behind_the_switch(compiled, pers):
    res, text = compiled
    names = [k for k in res if f"k_logits_f16xILi3ELi3ELb{pers}ELi0EE" in k]
    assert len(names) == 1, sorted(res)
    body = body_of(text, names[0])
    assert len([l for l in body if l.startswith("v_mfma_f32_32x32x16_f16")]) == 576
    assert not [l for l in body if "v_mfma_f32_16x16x32_f16" in l]
