"""Developer check (no GPU needed): the gfx950 kernels of two builds of libuvrt_hip.so, instruction for instruction.

    python tests/tools/compare_kernels.py <old libuvrt_hip.so> <new libuvrt_hip.so>

Extracts the gfx950 code objects from the .hip_fatbin section of both libraries (one uncompressed offload bundle per
translation unit), disassembles them with llvm-objdump -d and compares every kernel's instruction sequence (addresses,
encodings and comments dropped).  One line per kernel: identical / DIFFERENT / NEW / GONE and its instruction count."""
import subprocess, sys, re, os, struct, tempfile
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin') + os.sep
MAGIC=b'__CLANG_OFFLOAD_BUNDLE__'
def code_objects(lib, work):
    sec=os.path.join(work,'fatbin')
    subprocess.check_call([LLVM+'llvm-objcopy','--dump-section','.hip_fatbin='+sec,lib,os.path.join(work,'copy')])
    d=open(sec,'rb').read()
    outs=[]
    pos=d.find(MAGIC)
    if pos<0: raise SystemExit('no uncompressed offload bundle in '+lib+' (magic %r)'%d[:8])
    while pos>=0:
        n,=struct.unpack_from('<Q',d,pos+24)
        q=pos+32
        for _ in range(n):
            off,size,idl=struct.unpack_from('<QQQ',d,q); q+=24
            ident=d[q:q+idl].decode(); q+=idl
            if 'gfx950' in ident and size>0:
                f=os.path.join(work,'co%d.elf'%len(outs)); open(f,'wb').write(d[pos+off:pos+off+size]); outs.append(f)
        pos=d.find(MAGIC,pos+1)
    return outs
def kernels(lib):
    ks={}
    with tempfile.TemporaryDirectory() as w:
        for co in code_objects(lib,w):
            txt=subprocess.run([LLVM+'llvm-objdump','-d','--no-show-raw-insn','--no-leading-addr',co],capture_output=True,text=True,check=True).stdout
            cur=None
            for line in txt.splitlines():
                m=re.match(r'^(?:[0-9a-f]+ )?<([^>]+)>:$',line.strip())
                if m: cur=m.group(1); ks[cur]=[]; continue
                if cur is None or not line.strip(): continue
                ins=re.sub(r'\s*//.*$','',line.strip())
                if ins!='...': ks[cur].append(ins)
    return ks
a=kernels(sys.argv[1]); b=kernels(sys.argv[2])
dem=lambda n: subprocess.run(['c++filt',n],capture_output=True,text=True).stdout.strip()
for n in sorted(set(a)|set(b)):
    if n.endswith('.kd') or n.startswith('__'): continue
    if n not in a: print('NEW       %6d instr  %s'%(len(b[n]),dem(n)))
    elif n not in b: print('GONE      %6d instr  %s'%(len(a[n]),dem(n)))
    else: print('%-9s %6d instr  %s'%('identical' if a[n]==b[n] else 'DIFFERENT',len(a[n]),dem(n)))
