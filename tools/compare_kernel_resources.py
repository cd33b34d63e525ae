"""Compares the metadata of every kernel of two builds of libmtsamd.so -- a parent commit's and this tree's: VGPRs, SGPRs, AGPRs,
spilled registers, scratch, LDS and the size of the kernel-argument record, read from the code objects.  Prints which kernels of the
first library are missing from or differ in the second (a growth of the kernel-argument record alone is listed apart: the tail of
DScene), and the resources of the kernels only the second one has.  profiles/instance_resources.txt is its output.

    python tools/compare_kernel_resources.py PARENT/libmtsamd.so [THIS/libmtsamd.so]

Build the parent in a checkout of its own (python eradiate-kernel_amd/build.py there); no GPU is needed."""
import re, subprocess, sys, os, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
llvm = "/opt/rocm/lib/llvm/bin"
F=("vgpr_count","sgpr_count","agpr_count","private_segment_fixed_size","group_segment_fixed_size","kernarg_segment_size","vgpr_spill_count","sgpr_spill_count")
def kernels(lib):
    tmp=tempfile.mkdtemp()
    fat=os.path.join(tmp,"fat.bin")
    subprocess.run([llvm+"/llvm-objcopy","-O","binary","--only-section=.hip_fatbin",lib,fat],check=True)
    blob=open(fat,"rb").read(); magic=b"__CLANG_OFFLOAD_BUNDLE__"
    starts=[m.start() for m in re.finditer(re.escape(magic),blob)]
    out={}
    for k,o in enumerate(starts):
        part,co=os.path.join(tmp,"b%d.bin"%k),os.path.join(tmp,"b%d.co"%k)
        open(part,"wb").write(blob[o:starts[k+1] if k+1<len(starts) else len(blob)])
        subprocess.run([llvm+"/clang-offload-bundler","--unbundle","--type=o","--input="+part,"--targets=hipv4-amdgcn-amd-amdhsa--gfx950","--output="+co],check=True,stdout=subprocess.DEVNULL,stderr=subprocess.DEVNULL)
        notes=subprocess.run([llvm+"/llvm-readelf","--notes",co],check=True,capture_output=True,text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            block="- .agpr_count"+block
            name=re.search(r"\.name:\s+(\S+)",block).group(1)
            out[name]={f:int(re.search(r"\.%s:\s+(\d+)"%f,block).group(1)) for f in F}
    return out,len(starts)
a, na = kernels(sys.argv[1]); b, nb = kernels(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "eradiate-kernel_amd", "libmtsamd.so"))
print("bundles: parent %d, this commit %d; kernels: parent %d, this commit %d"%(na,nb,len(a),len(b)))
missing=[k for k in a if k not in b]
print("pre-existing kernel symbols missing in this commit: %d"%len(missing)); [print("  ",k) for k in missing]
diff=0
for k in sorted(a):
    if k in b:
        d={f:(a[k][f],b[k][f]) for f in F if a[k][f]!=b[k][f]}
        only_kernarg = set(d)=={"kernarg_segment_size"}
        if d and not only_kernarg: diff+=1; print("DIFFERS",k,d)
ks={ (b[k]["kernarg_segment_size"]-a[k]["kernarg_segment_size"]) for k in a if k in b}
print("kernarg size differences (the DScene tail):",sorted(ks))
print("pre-existing kernels whose VGPRs / SGPRs / AGPRs / scratch / LDS / spills differ: %d of %d"%(diff,len(a)))
print("new kernels (VGPRs / SGPRs / spilled VGPRs / spilled SGPRs / scratch B / LDS B / kernarg B):")
for k in sorted(b):
    if k not in a:
        v=b[k]; dem=subprocess.run(["c++filt",k],capture_output=True,text=True).stdout.strip().split("(")[0]
        print("  %s: %d / %d / %d / %d / %d / %d / %d"%(dem,v["vgpr_count"],v["sgpr_count"],v["vgpr_spill_count"],v["sgpr_spill_count"],v["private_segment_fixed_size"],v["group_segment_fixed_size"],v["kernarg_segment_size"]))
