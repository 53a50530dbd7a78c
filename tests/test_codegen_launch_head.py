"""The launch head of the C2 hot kernels in the emitted code (CPU: hipcc cross-compiles gfx950 assembly, as
tests/test_codegen.py does).

A one-wave launch cannot compute before its first operand DMA (`buffer_load_dwordx4 ... lds`) lands, so what a wave
runs before issuing it is on the critical path of every launch (DESIGN.md §3 'Launch head'). The kernels read the
first 64 bytes of their argument struct (the hot line, kernels.h) as one batch of scalar loads and compute only the
tile origin, the extents and the lanes' offsets before the DMA. Pinned here, on the listing from the function label
to the first LDS-DMA (every block laid out in between counts, taken or not):

  * kernel-argument load rounds -- `s_waitcnt` with lgkmcnt that retire at least one `s_load*` from the
    kernel-argument pointer (s[0:1] or a copy of it): at most 3, one for the hot line plus at most two for the
    probed path's dependent load under its branch. The parent commit had 6, 5, 5 and 8 (some of them not yet waited
    for at the DMA);
  * instructions ahead of the DMA: below a constant per kernel, the achieved count rounded up to the next 25
    (the parent commit: 433, 288, 272 and 328);
  * the loads ahead of the first wait read inside the hot line only, and no load ahead of the DMA reads at or past
    the end of the struct, where the hidden arguments (the grid size) start.
"""

import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "f5-tts_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=fast-honor-pragmas",
         "-mllvm", "-disable-promote-alloca-to-lds=1", "--cuda-device-only", "-S"]

GEMM_ARGS_BYTES, ATTN_ARGS_BYTES, HOT_LINE = 304, 120, 64
# bf16, write-through variants (the C2 launches): (source, mangled-name pattern, struct bytes, instruction bound,
# the parent commit's instruction count)
KERNELS = {
    "out-proj/ffn2": ("gemm_bf16_a.hip", r"gemm_kernelIDF16bLi9ELi64ELi128ELi2ELi2ELi3ELb1ELi128ELi16ELb0ELb0EE",
                      GEMM_ARGS_BYTES, 150, 433),
    "qkv": ("gemm_bf16_a.hip", r"gemm_kernelIDF16bLi7ELi192ELi128ELi2ELi2ELi2ELb1ELi128ELi16ELb0ELb0EE",
            GEMM_ARGS_BYTES, 125, 288),
    "ffn1": ("gemm_bf16_a.hip", r"gemm_kernelIDF16bLi2ELi128ELi128ELi2ELi2ELi2ELb1ELi128ELi16ELb0ELb0EE",
             GEMM_ARGS_BYTES, 125, 272),
    "attention": ("attention.hip", r"attn16_kernelIDF16bLb1ELi8ELb0ELb1ELb0ELb0EE", ATTN_ARGS_BYTES, 125, 328),
}
MAX_ROUNDS = 3

_cache = {}


def _asm(src, tmp_path_factory):
    if src not in _cache:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        out = tmp_path_factory.mktemp("head") / (src + ".s")
        subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True,
                       timeout=600)
        _cache[src] = out.read_text().splitlines()
    return _cache[src]


def _function(lines, pattern):
    """The instruction lines of the one function whose mangled name matches."""
    found, cur = {}, None
    for ln in lines:
        m = re.match(r"^(_Z\S+):(\s|$)", ln)
        if m and re.search(pattern, m.group(1)):
            cur = m.group(1)
            found[cur] = []
            continue
        if cur and (ln.startswith("\t.size\t" + cur) or ln.startswith(".Lfunc_end")):
            cur = None
        elif cur:
            found[cur].append(ln.strip())
    assert len(found) == 1, (pattern, list(found))
    return next(iter(found.values()))


def _head(body):
    """Instructions from the function label to the first LDS-DMA (labels, directives and comments dropped)."""
    ins = []
    for ln in body:
        if not ln or ln.startswith(";") or ln.startswith(".") or re.match(r"^\S+:", ln):
            continue
        if ln.startswith("buffer_load_dwordx4") and ln.endswith(" lds"):
            return ins
        ins.append(ln)
    raise AssertionError("no LDS-DMA in the kernel")


def _sregs(op):
    m = re.match(r"s\[(\d+):(\d+)\]$", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"s(\d+)$", op)
    return {int(m.group(1))} if m else set()


def _karg_loads(ins):
    """[(index, offset, bytes)] of the s_load* from the kernel-argument pointer -- s[0:1], or a register pair it was
    copied to and that nothing has overwritten since -- and the indices of the lgkmcnt waits that retire one."""
    bases = {"s[0:1]"}
    loads, waits, pending = [], [], 0
    for i, ln in enumerate(ins):
        ops = [o.strip() for o in ln.split(None, 1)[1].split(",")] if " " in ln else []
        m = re.match(r"s_load_dword(x(\d+))? \S+, (s\[\d+:\d+\]), (0x[0-9a-f]+|\d+)$", ln)
        if m and m.group(3) in bases:
            loads.append((i, int(m.group(4), 0), 4 * int(m.group(2) or 1)))
            pending += 1
        elif ln.startswith("s_waitcnt") and "lgkmcnt" in ln:
            if pending:
                waits.append(i)
            pending = 0
        if ln.startswith("s_mov_b64") and len(ops) == 2 and ops[1] in bases:
            bases.add(ops[0])
        elif ops and not ln.startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop")):
            written = _sregs(ops[0])
            bases = {b for b in bases if b == "s[0:1]" or not (_sregs(b) & written)}
    return loads, waits


@pytest.mark.parametrize("name", list(KERNELS))
def test_launch_head(name, tmp_path_factory):
    src, pattern, struct_bytes, bound, parent = KERNELS[name]
    ins = _head(_function(_asm(src, tmp_path_factory), pattern))
    loads, waits = _karg_loads(ins)
    first = [(off, nb) for i, off, nb in loads if i < waits[0]]
    print(f"[launch-head] {name}: {len(waits)} kernel-argument load rounds, {len(ins)} instructions before the first "
          f"LDS-DMA (parent {parent}); first batch (offset, bytes) {first}")
    assert waits and loads and loads[0][0] < waits[0], "the hot line is loaded first"
    assert len(waits) <= MAX_ROUNDS, (name, len(waits), [ins[i] for i, _, _ in loads])
    assert bound < parent and len(ins) <= bound, (name, len(ins), bound)
    assert all(off + nb <= HOT_LINE for off, nb in first), (name, first)
    assert all(off < struct_bytes for _, off, _ in loads), (name, "a hidden-argument load ahead of the DMA", loads)
