"""Resource guards on the compiled gfx950 kernels (no GPU needed: hipcc cross-compiles to assembly).

A kernel with a private segment (scratch: register spills, or a local object the compiler could not keep in registers) pays a scratch
set-up on every queue that first runs it and makes every dispatch depend on the scratch allocation — measured in round 2 as a 1.5 ms
first launch of k_quadtree on a new stream and an 11x slower kernel under counter collection.  Every kernel of the library must
therefore report `.amdhsa_private_segment_fixed_size 0`."""
import re
from concurrent.futures import ThreadPoolExecutor

from tests import abi_util


@abi_util.needs_hipcc
def test_no_kernel_uses_scratch_memory():
    from orb_slam3_modified_amd.build import SOURCES
    with ThreadPoolExecutor(len(SOURCES)) as ex:
        scratch = dict(zip(SOURCES, ex.map(abi_util.kernel_scratch, SOURCES)))
    assert sum(len(ks) for ks in scratch.values()) >= 30
    bad = [(src, k, v) for src, ks in scratch.items() for k, v in ks.items() if v != 0]
    assert not bad, bad
    # the kernels that stage a tile / rectangle / window fill it by LDS-DMA: the builtin must have survived the compiler
    dma = {}   # kernel symbol -> number of LDS-DMA loads in its body
    for src in SOURCES:
        body = None
        for line in abi_util.device_asm(src).splitlines():
            m = re.match(r"(_Z\w+):\s*", line)
            if m:
                body = m.group(1)
            if body and "global_load_lds_dword" in line:
                dma[body] = dma.get(body, 0) + 1
    for frag in ("k_fast_cellsILi128ELi64ELb1", "k_fast_blurILi64ELb1", "k_resize", "k_blur7", "k_describeILi4ELb1ELb0"):
        hit = [k for k in dma if frag in k]
        assert hit, (frag, sorted(dma))
