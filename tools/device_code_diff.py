"""Are two gfx950 code objects the same device code?   usage: python tools/device_code_diff.py a.o b.o
Compares the sorted kernel symbol lists, every kernel's instruction stream (addresses relative to the kernel's start, so
the order in which kernels are emitted does not matter) and every kernel's metadata note (registers, LDS, arguments).
The objects come from the Makefile's flags plus `--offload-device-only --no-gpu-bundle-output -cuid=<fixed> -c`; with
the compilation-unit id fixed, a host-only change leaves the whole file's checksum unchanged as well
(profiles/edge_dispatch_refactor.txt)."""
import re, subprocess, sys, hashlib
OBJDUMP='/opt/rocm/lib/llvm/bin/llvm-objdump'; READELF='/opt/rocm/lib/llvm/bin/llvm-readelf'
def funcs(path):
    out=subprocess.run([OBJDUMP,'-d','--no-show-raw-insn',path],capture_output=True,text=True,check=True).stdout
    res={}; cur=None; base=0
    for line in out.splitlines():
        m=re.match(r'^([0-9a-f]+) <(.+)>:$',line)
        if m:
            cur=m.group(2); base=int(m.group(1),16); res[cur]=[]; continue
        if cur is None or not line.strip() or line.strip() == '...': continue      # (zero padding behind a function)
        # "   insn operands   // 000000001234: " style or leading address
        m=re.match(r'^\s*([0-9a-f]+):\s*(.*)$',line)
        if m: addr=int(m.group(1),16); txt=m.group(2)
        else:
            m=re.match(r'^\s*(.*?)\s*//\s*([0-9A-Fa-f]+):.*$',line)
            if not m: res[cur].append(line.strip()); continue
            addr=int(m.group(2),16); txt=m.group(1)
        # branch targets: "<sym+0x..>" keep (function relative); absolute numbers in comments dropped
        res[cur].append('%x %s'%(addr-base,txt))
    return res
def meta(path):
    out=subprocess.run([READELF,'--notes',path],capture_output=True,text=True,check=True).stdout
    ks={}; cur=[]
    blocks=re.split(r'\n\s+- \.agpr_count',out)
    for b in blocks[1:]:
        b='.agpr_count'+b
        name=re.search(r'\.name:\s+(\S+)',b).group(1)
        b=b.split('\namdhsa.target')[0].split('\namdhsa.printf')[0]
        ks[name]=re.sub(r'\s+','\n',b.strip())
    return ks
a,b=sys.argv[1],sys.argv[2]
fa,fb=funcs(a),funcs(b); ma,mb=meta(a),meta(b)
ok=True
if sorted(fa)!=sorted(fb): ok=False; print('SYMBOLS DIFFER', sorted(set(fa)^set(fb))[:6])
for k in sorted(set(fa)&set(fb)):
    if fa[k]!=fb[k]:
        ok=False; print('CODE DIFFERS',k,len(fa[k]),len(fb[k]))
if sorted(ma)!=sorted(mb): ok=False; print('KERNEL LIST DIFFERS', sorted(set(ma)^set(mb))[:6])
for k in sorted(set(ma)&set(mb)):
    if ma[k]!=mb[k]: ok=False; print('METADATA DIFFERS',k)
h=hashlib.sha256('\n'.join(k+'\n'+'\n'.join(fa[k]) for k in sorted(fa)).encode()).hexdigest()
print(('IDENTICAL' if ok else 'DIFFERENT'), len(fa),'functions',len(ma),'kernels','sorted-disassembly sha256',h)
