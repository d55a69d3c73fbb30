"""Build-time gate for the 256-key dK/dV kernel (csrc/usp_flash_bwd64u.hip).  No GPU: hipcc cross-compiles gfx950.

The kernel owns the accumulator file by hand: its 16 accumulators ARE a[0:255], named in the text of its asm MFMAs, and hipcc is
kept away from them by clobber lists alone.  What that rests on is checked here on a fresh compile, so that another compiler
fails loudly instead of corrupting accumulators:
- no instruction but the asm MFMAs and the epilogue's v_accvgpr_read names an accumulator register (no v_accvgpr_write / _mov: hipcc
  uses no AGPR as a home or a spill slot);
- the tile loops (the loops of 128 MFMAs) carry no scratch traffic, no v_accvgpr instruction, no v_readlane / v_writelane;
- tools/mfma_hazards.py finds nothing in any instantiation -- including a VALU write in front of an MFMA's SrcC where SrcC is
  also D (the chains START from row constants that hipcc copies with v_mov): the rule has a planted-hazard test of its own below.
"""
import collections
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "long-context-attention_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("dkdv64u") / "usp_flash_bwd64u.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", f"-I{os.path.join(ROOT, 'include')}",
           "--cuda-device-only", "-S", os.path.join(CSRC, "usp_flash_bwd64u.hip"), "-o", out]      # the flags of csrc/Makefile that shape device code
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _kernels(path):
    """{mangled name: (instructions, {label: index of its first instruction})} of the functions of a .s file."""
    out, cur = {}, None
    for l in open(path).read().split("\n"):
        m = re.match(r"^(_Z\S*):", l)
        if m:
            cur = m.group(1)
            out[cur] = ([], {})
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
        if cur is None:
            continue
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            out[cur][1][m.group(1)] = len(out[cur][0])
            continue
        t = l.split(";")[0].strip()
        if t and not t.startswith((".", "//")):
            out[cur][0].append(t)
    return {n: v for n, v in out.items() if any("v_mfma" in i for i in v[0])}


def _loops(ins, labels):
    """The innermost loops (backward branches whose body holds no later loop head) as instruction lists."""
    rng = []
    for i, t in enumerate(ins):
        if t.startswith(("s_cbranch", "s_branch")):
            tgt = t.split()[-1]
            if tgt in labels and labels[tgt] <= i:
                rng.append((labels[tgt], i))
    for a, b in rng:
        if not any(a < a2 and b2 <= b for a2, b2 in rng):
            yield ins[a:b + 1]


def test_accumulator_registers_are_touched_by_the_asm_alone(asm):
    ks = _kernels(asm)
    assert len(ks) == 4, sorted(ks)                  # bf16 / fp16 x causal / full
    for name, (ins, _) in ks.items():
        reads = 0
        for t in ins:
            if not re.search(r"\ba(\d+|\[\d+:\d+\])(,|$|\s)", t):
                continue
            op = t.split()[0]
            assert op.startswith("v_mfma") or op == "v_accvgpr_read_b32", f"{name}: {t}"
            reads += op == "v_accvgpr_read_b32"
        assert reads == 256, (name, reads)           # the epilogue: 16 accumulators x 16 registers, once each
        assert not any(t.startswith(("v_accvgpr_write", "v_accvgpr_mov")) for t in ins), name


def test_tile_loops_carry_no_scratch_and_no_register_file_copies(asm):
    for name, (ins, labels) in _kernels(asm).items():
        tile = [b for b in _loops(ins, labels) if sum("v_mfma" in t for t in b) == 128]
        assert len(tile) >= (2 if "Lb1E" in name else 1), (name, len(tile))          # causal: a masked and a plain instance
        for b in tile:
            c = collections.Counter(t.split()[0] for t in b)
            bad = {k: v for k, v in c.items() if k.startswith(("scratch_", "v_accvgpr", "v_readlane", "v_writelane"))}
            assert not bad, (name, bad)
            assert len(b) <= 12 * 128, (name, len(b))                                # (the masked instance runs at 8 - 9 per MFMA)


def test_no_software_visible_mfma_hazard(asm):
    import mfma_hazards as H
    names = H.kernels_in(asm)
    assert len(names) == 4, names
    for n in names:
        found = []
        assert H.check(asm, n, out=found.append) == 0, f"{n}:\n" + "\n".join(found[:10])


def test_the_checker_sees_a_valu_write_in_front_of_src_c_that_is_also_d(tmp_path):
    """What the first build of this kernel did: the chain's start constants copied into its accumulator one and two instructions in
    front of the chain's first MFMA (C = D = that accumulator).  Two wait states in between are clean."""
    import mfma_hazards as H
    s = tmp_path / "c.s"
    s.write_text("\n".join([
        "_Z1kv:",
        "\tv_mov_b64_e32 v[50:51], v[34:35]",
        "\tv_mov_b64_e32 v[48:49], v[32:33]",
        "\tv_mfma_f32_32x32x16_bf16 v[48:63], v[0:3], v[92:95], v[48:63]",
        "\ts_nop 15",
        "\ts_endpgm",
        ".Lfunc_end0:", ""]))
    found = []
    assert H.check(str(s), "_Z1kv", out=found.append) == 2 and all(x.startswith("A:") for x in found), found
    ok = tmp_path / "ok.s"
    ok.write_text("\n".join([
        "_Z1ov:",
        "\tv_mov_b64_e32 v[50:51], v[34:35]",
        "\tv_mov_b64_e32 v[48:49], v[32:33]",
        "\ts_nop 1",
        "\tv_mfma_f32_32x32x16_bf16 v[48:63], v[0:3], v[92:95], v[48:63]",
        "\tv_mfma_f32_32x32x16_bf16 v[48:63], v[4:7], v[96:99], v[48:63]",          # the accumulate chain itself stays exempt
        "\ts_nop 15",
        "\ts_endpgm",
        ".Lfunc_end0:", ""]))
    assert H.check(str(ok), "_Z1ov", out=found.append) == 0, found
