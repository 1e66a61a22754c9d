"""The chain kernel fits its registers without scratch -- read from the BUILT library, no GPU.

The 64 x 512 tile of the general split kernel stands at 244 of 256 VGPRs, and fused_split_chain_kernel keeps more alive across a layer
(bt_fused_split.h: member_tid, UCAP, the xm 0 arm's late weight loads are there for that). A compiler that decides otherwise would spill
silently: nothing computes differently, the launch only gets slower. So the code objects inside libbtorch_hip.so are taken out of its
.hip_fatbin bundles and the kernel metadata (llvm-readelf --notes: what the loader itself reads) of both chain instantiations is held to
no private segment, no spilled VGPR and at most 256 VGPRs."""
import os
import re
import shutil
import struct
import subprocess

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(lib_path, needle):
    """The gfx950 code objects of the library's offload bundles that contain ``needle``."""
    data = open(lib_path, "rb").read()
    for m in re.finditer(MAGIC, data):
        p = m.start()
        (n,) = struct.unpack_from("<Q", data, p + len(MAGIC))
        q = p + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size and needle in data[p + off:p + off + size]:
                yield data[p + off:p + off + size]


def _kernel_notes(elf_bytes, tmp_path):
    """name -> {field: int} of every kernel in the code object's AMDGPU metadata note."""
    tool = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(tool), "llvm-readelf (ROCm's LLVM) is needed to read the kernels' metadata"
    path = os.path.join(tmp_path, "chain.co")
    with open(path, "wb") as f:
        f.write(elf_bytes)
    out = subprocess.run([tool, "--notes", path], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in out.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", "  .agpr_count:" + block, flags=re.M)}
    return kernels


def test_chain_instantiations_have_no_scratch(tmp_path):
    from bayesian_torch_amd import _lib
    objs = list(_code_objects(_lib.LIB_PATH, b"fused_split_chain_kernel"))
    assert len(objs) == 1, "one translation unit instantiates the chain kernel"
    notes = {k: v for k, v in _kernel_notes(objs[0], str(tmp_path)).items() if "fused_split_chain_kernel" in k}
    assert sorted(re.search(r"ILi64ELi512ELi3ELi4ELi(\d)E", k).group(1) for k in notes) == ["0", "3"], sorted(notes)      # xm 0 and xm 3
    for name, n in notes.items():
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (name, n)
        assert n["vgpr_count"] + n["agpr_count"] <= 256, (name, n)
        assert n["max_flat_workgroup_size"] == 512, (name, n)
