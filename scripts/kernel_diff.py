"""kernel_diff.py PARENT.co NEW.co: are the kernels two builds share the same machine code?  For every FUNC symbol of two gfx950 code objects
(llvm-objdump --offloading <obj>.o extracts one per translation unit) the bytes of [st_value, st_value + st_size) in .text are compared.
profiles/retired_switches_kernel_diff.txt was made with it."""
import subprocess, sys, re
RE='/opt/rocm/llvm/bin/llvm-readelf'
def kernels(co):
    data=open(co,'rb').read()
    secs=subprocess.run([RE,'-SW',co],capture_output=True,text=True).stdout
    m=re.search(r'\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)',secs)
    addr,off=int(m.group(1),16),int(m.group(2),16)
    out={}
    for l in subprocess.run([RE,'-sW',co],capture_output=True,text=True).stdout.splitlines():
        f=l.split()
        if len(f)>=8 and f[3]=='FUNC':
            v,sz=int(f[1],16),int(f[2]); out[f[7]]=data[off+v-addr:off+v-addr+sz]
    return out
a,b=kernels(sys.argv[1]),kernels(sys.argv[2])
print('parent',len(a),'new',len(b),'removed',len(set(a)-set(b)),'added',len(set(b)-set(a)))
same=[k for k in b if k in a and a[k]==b[k]]; diff=[k for k in b if k in a and a[k]!=b[k]]
print('identical',len(same),'differ',len(diff))
for k in diff: print(' DIFF',k[:100],len(a[k]),len(b[k]))
print('bytes parent',sum(map(len,a.values())),'new',sum(map(len,b.values())))
