"""Medians and the parent's spread (max - min of its three runs) from the raw
outputs in speed/ (w<workload>_<parent|new>_<run>.txt), as markdown.

    python speed_table.py speed
"""
import glob,re,statistics as st,json,sys
D=sys.argv[1]
names={1:'RS --batch 16384 --pool',2:'RS --algo msa --p 0.002 --iters 50 --batch 65536 --pool',3:'RS --p 0.004 --iters 50 --batch 65536 --chunk 8192',4:'RS --algo msa --p 0.002 --iters 50 --batch 65536 --chunk 8192',5:'RS --fixed --batch 16384',6:'"random (4,32)" --batch 16384',7:'"random (4,32)" --fixed --batch 16384'}
def rows(f):
    out={}
    for l in open(f):
        m=re.match(r'(.{32}) +(\d+) +(\d+) +(\d+) +(\d+) +(\d+) +(\S+) +([\d.]+) +([\d.]+) +([\d.]+) +([\d.]+) +([\d.]+) +([\d.]+) +([\d.]+)',l)
        if m: out[m.group(1).strip()]=(m.group(7),float(m.group(8)),float(m.group(12)),float(m.group(13)))
    return out
bad=0
for w in range(1,8):
    P=[rows(f'{D}/w{w}_parent_{i}.txt') for i in (1,2,3)]; N=[rows(f'{D}/w{w}_new_{i}.txt') for i in (1,2,3)]
    print(f'\n### `--only {names[w]}`\n')
    print('| code | path | cw/s parent (median, spread) | cw/s new | check µs parent (spread) | check µs new | variable µs parent (spread) | variable µs new | within |')
    print('|---|---|---|---|---|---|---|---|---|')
    for c in P[0]:
        def col(R,k): return [r[c][k] for r in R]
        res=[]
        ok=True
        cells=[]
        for k,hi in ((1,True),(2,False),(3,False)):
            p=col(P,k); n=col(N,k); pm=st.median(p); nm=st.median(n); sp=max(p)-min(p)
            good = nm>=pm-sp if hi else nm<=pm+sp
            ok&=good
            cells+= [f'{pm:.1f} ({sp:.1f})', f'{nm:.1f}'+('' if good else ' **!**')]
        if not ok and not c.startswith('DNA') and 'RS(9,72,8)' not in c: bad+=1
        print(f'| {c} | {P[0][c][0]} | '+' | '.join(cells)+f' | {"yes" if ok else "NO"} |')
print('\n### `bench.py --gpus 1`\n')
pv=[json.loads(open(f'{D}/w8_parent_{i}.txt').read().strip().split('\n')[-1]) for i in (1,2,3)]
nv=[json.loads(open(f'{D}/w8_new_{i}.txt').read().strip().split('\n')[-1]) for i in (1,2,3)]
p=[x['value'] for x in pv]; n=[x['value'] for x in nv]
print('parent value', p, 'median', st.median(p), 'spread', round(max(p)-min(p),2))
print('new value   ', n, 'median', st.median(n), 'ok' if st.median(n)>=st.median(p)-(max(p)-min(p)) else 'NOT OK')
print(sorted(pv[0].keys()))
print('\n### kernels whose register counts moved and that no workload above reaches (w9)\n')
print('| case | path | cw/s parent (median, spread) | cw/s new | check µs parent (spread) | check µs new | variable µs parent (spread) | variable µs new | launches check/variable parent, new | within |')
print('|---|---|---|---|---|---|---|---|---|---|')
def rows9(f):
    out={}
    for l in open(f):
        m=re.match(r'(.+?)\s+(res|grp|fix) cw/s\s+([\d.]+) it/cw\s+[\d.]+ chk us\s+([\d.]+) var us\s+([\d.]+) launches (\S+)',l)
        if m: out[m.group(1)]=(m.group(2),float(m.group(3)),float(m.group(4)),float(m.group(5)),m.group(6))
    return out
P=[rows9(f'{D}/w9_parent_{i}.txt') for i in (1,2,3)]; N=[rows9(f'{D}/w9_new_{i}.txt') for i in (1,2,3)]
for c in P[0]:
    ok=True; cells=[]
    for k,hi in ((1,True),(2,False),(3,False)):
        p=[r[c][k] for r in P]; n=[r[c][k] for r in N]; pm=st.median(p); nm=st.median(n); sp=max(p)-min(p)
        good = nm>=pm-sp if hi else nm<=pm+sp
        ok&=good
        cells+=[f'{pm:.1f} ({sp:.1f})', f'{nm:.1f}'+('' if good else ' **!**')]
    print(f'| {c} | {P[0][c][0]} | '+' | '.join(cells)+f' | {P[0][c][4]}, {N[0][c][4]} | {"yes" if ok else "NO"} |')
