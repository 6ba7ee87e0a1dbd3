"""Compare two device assembly listings of csrc/engine.hip (hipcc
--cuda-device-only -S with the Makefile's flags; parent, new) kernel by
kernel: the text of each kernel up to its .Lfunc_end, comments and blank
lines dropped, local label numbers and the kernel's own name normalised, the
renamed kernels matched to their predecessors.

    python compare_asm.py parent_engine.s new_engine.s
"""
import re,sys,subprocess
def funcs(p):
    d={};cur=None
    for l in open(p):
        m=re.match(r'^(_Z\S+):\s*(;.*)?$',l)
        if m: cur=m.group(1); d[cur]=[]; continue
        if cur is not None:
            if l.startswith('.Lfunc_end'): cur=None; continue
            t=l.strip()
            if not t or t.startswith(';'): continue
            l=re.sub(r'Header=BB\d+_', 'Header=BBN_', re.sub(r'\.L(BB|JTI|tmp|func_begin|func_end|CPI)\d+_?', r'.L\1N_', l))
            l=re.sub(r';.*','',l).rstrip()
            d[cur].append(l.replace(cur,'SELF'))
    return d
def dem(d):
    names=list(d)
    out=subprocess.run(['c++filt'],input='\n'.join(names),capture_output=True,text=True).stdout.split('\n')
    r={}
    for n,o in zip(names,out):
        o=re.sub(r'\(.*','',o).replace('ldpc::dev::','').replace('void ','')
        o=re.sub(r"k_check_bp_gr<(\d+)>",r"k_check_gr<false, \1>",o); o=re.sub(r"k_check_msa_gr<(\d+)>",r"k_check_gr<true, \1>",o)
        o=re.sub(r"k_var_bp_gr<(\d+)>",r"k_var_gr<false, \1>",o); o=re.sub(r"k_var_msa_gr<(\d+)>",r"k_var_gr<true, \1>",o)
        r[o]=d[n]
    return r
a=dem(funcs(sys.argv[1])); b=dem(funcs(sys.argv[2]))
def canon(ls):
    # commutative fp64 multiply / add: operand order is the compiler's choice
    out=[]
    for l in ls:
        m=re.match(r'(\s+v_(?:mul|add)_f64 \S+, )(\S+), (\S+)$',l)
        if m and not any(x in l for x in ('-','|','neg','abs')):
            a_,b_=sorted([m.group(2),m.group(3)]); l=m.group(1)+a_+', '+b_
        out.append(l)
    return out
same=[];diff=[];comm=[]
for n in sorted(set(a)&set(b)):
    (same if a[n]==b[n] else comm if canon(a[n])==canon(b[n]) else diff).append(n)
print('same',len(same),'same but for the operand order of commutative fp64 mul/add',len(comm),'differ',len(diff))
for n in comm: print('  COMMUTED',n)
for n in diff: print('  DIFFERS',n,len(a[n]),'->',len(b[n]))
fam={}
for n in same: fam.setdefault(n.split('<')[0],[0,0,0])[0]+=1
for n in comm: fam.setdefault(n.split('<')[0],[0,0,0])[1]+=1
for n in diff: fam.setdefault(n.split('<')[0],[0,0,0])[2]+=1
print('\nby kernel family: identical / operand order only / different')
for f in sorted(fam): print(f'  {f:28s} {fam[f][0]:4d} {fam[f][1]:4d} {fam[f][2]:4d}')
