"""Launch counts per kernel class of three deterministic decodes; run with the tree's root as argv[1]."""
import json, os, sys
import numpy as np
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.join(root, "dna-ldpc-codes_amd"))
import ldpc_amd as L
import synth
cw = synth.load_codewords()
G = L.Graph(synth.PCHK)
N = G.N
d_cw = L.DeviceBuffer(0, cw.nbytes); d_cw.upload(cw)
table = np.arange(-128, 128, dtype=np.float64) * synth.LLR_UNIT
out = {"lib": L.LIB_PATH}

def run(name, eng, d_in, B, max_iter):
    d_h, d_i, d_v = L.DeviceBuffer(0, B * N), L.DeviceBuffer(0, B * 4), L.DeviceBuffer(0, B)
    eng.profile(0)
    eng.decode_codes(d_in.at(0), table, L.IN_LLR, B, max_iter, d_h.at(0), None, L.POST_LLR, d_i.at(0), d_v.at(0))
    eng.sync()
    st = eng.stats()
    it = d_i.download(np.empty(B, np.int32))
    out[name] = {"launches": {k: v["launches"] for k, v in st.items()}, "iters_sum": int(it.sum()),
                 "cap": eng.cap, "flags": eng.flags}

for name, algo, B, p, mi in (("headline_bp_B1000", "bp", 1000, 0.02, 50), ("config5_msa_B10000", "msa", 10000, 0.002, 50)):
    eng = L.Engine(G, 0, algo)
    d_in = L.DeviceBuffer(0, B * N)
    eng.gen_bsc_codes(d_in.at(0), 0, B, d_cw.at(0), len(cw), 2026, p)
    run(name, eng, d_in, B, mi)
    eng.close()
llr = synth.dna_like_llrs(cw, seed=0)
k = np.rint(llr / synth.LLR_UNIT).astype(np.int8)
B = len(k)
eng = L.Engine(G, 0, "bp", chunk=B)
d_in = L.DeviceBuffer(0, B * N); d_in.upload(np.ascontiguousarray(k))
run("dna272_bp200", eng, d_in, B, 200)
eng.close()
print(json.dumps(out))
