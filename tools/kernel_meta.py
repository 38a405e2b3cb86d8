#!/usr/bin/env python3
"""Per-kernel code-object metadata of two builds side by side (no GPU needed): the table of profiles/elu_kernels.txt.

    python tools/kernel_meta.py PARENT_BUILD_DIR TREE_BUILD_DIR [UNIT ...]      (units default: gemm gemm_x3 kernels)

For every UNIT.hip.o of both ppo.c_amd/build directories: the gfx950 code object is taken out of the object file's
.hip_fatbin section (objcopy, clang-offload-bundler --unbundle), its AMDGPU metadata note read (llvm-readelf --notes),
and per kernel (vgpr, agpr, sgpr, scratch bytes, static LDS bytes, vgpr spills, sgpr spills) printed: "same" where the
two builds agree, "DIFF parent -> tree" where they do not, "NEW" / "GONE" for kernels only one build has.  A parent
whose tiled GEMM kernels still end in `bool TH` is matched to the activation kind HA: false = 0, true = 2."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin")
FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
          ".vgpr_spill_count", ".sgpr_spill_count"]


def meta(obj):
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fb,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        blk = ".agpr_count" + blk
        d = {f: re.search(re.escape(f) + r":\s+(\S+)", blk).group(1) for f in FIELDS + [".name"]}
        name = subprocess.run(["c++filt", d[".name"]], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(.*\)$", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))
        out[name] = tuple(int(d[f]) for f in FIELDS)
    return out


def kind_of_flag(name):
    if re.match(r"gemm_(f32|x3)_kernel<", name):
        name = re.sub(r", false>$", ", 0>", re.sub(r", true>$", ", 2>", name))
    return name


def main():
    parent, tree = sys.argv[1], sys.argv[2]
    print("%-100s %s" % ("kernel", "(vgpr, agpr, sgpr, scratch, lds, vspill, sspill)"))
    for unit in sys.argv[3:] or ["gemm", "gemm_x3", "kernels"]:
        p = {kind_of_flag(k): v for k, v in meta(os.path.join(parent, unit + ".hip.o")).items()}
        t = meta(os.path.join(tree, unit + ".hip.o"))
        print(f"== {unit}.hip: {len(p)} kernels in the parent, {len(t)} in the tree")
        for k in sorted(set(p) | set(t)):
            if k in p and k in t:
                print("%-100s %s %s" % (k, "same" if p[k] == t[k] else "DIFF %s ->" % (p[k],), t[k]))
            else:
                print("%-100s %s %s" % (k, "NEW " if k in t else "GONE", t.get(k, p.get(k))))


if __name__ == "__main__":
    main()
