"""Compare two tables of tools/resources.py (parent, new) by kernel name, the
renamed kernels matched to their predecessors.  Lists every kernel whose
numbers moved; WORSE marks more scratch or less occupancy.

    python compare_resources.py resources_parent.txt resources_new.txt
"""
import re,sys
def load(p):
    d={}
    for ln in open(p):
        m=re.match(r"(\S.*?)\s+VGPR\s+(\d+) AGPR\s+(\d+) SGPR\s+(\d+) scratch\s+(\d+) occ (\d+)",ln)
        if not m: print("??",ln); continue
        n=m.group(1)
        n=re.sub(r"k_check_bp_gr<(\d+)>",r"k_check_gr<false, \1>",n)
        n=re.sub(r"k_check_msa_gr<(\d+)>",r"k_check_gr<true, \1>",n)
        n=re.sub(r"k_var_bp_gr<(\d+)>",r"k_var_gr<false, \1>",n)
        n=re.sub(r"k_var_msa_gr<(\d+)>",r"k_var_gr<true, \1>",n)
        assert n not in d, n
        d[n]=tuple(map(int,m.groups()[1:]))
    return d
a=load(sys.argv[1]); b=load(sys.argv[2])
print("kernels:", len(a), len(b))
print("only parent:",sorted(set(a)-set(b)))
print("only new:",sorted(set(b)-set(a)))
for n in sorted(set(a)&set(b)):
    if a[n]!=b[n]:
        bad = b[n][3]>a[n][3] or b[n][4]<a[n][4]
        print(f"{n:55s} VGPR {a[n][0]}->{b[n][0]} SGPR {a[n][2]}->{b[n][2]} scratch {a[n][3]}->{b[n][3]} occ {a[n][4]}->{b[n][4]}", "  <== WORSE" if bad else "")
