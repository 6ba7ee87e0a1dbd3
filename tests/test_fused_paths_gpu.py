"""The fused row block's two paths (k_var_bp_fused): a tile without a
refilled, finished or last lane takes the plain path (a rolling window of
columns in flight per wave), every other tile the path with all arms, one
column at a time.  Nothing a codeword computes changes: every case equals the
oracle and the schedule without the flag bit for bit -- hard bits, iteration
counts, valid flags and the posterior ratio's bytes.

Codes, inputs and the Case helper are those of test_fused_rowblock_gpu; two
lattice inputs are added: `noisy` (every row a BSC with p = 0.02: the lanes
of a tile start together and, up to the few early exits, reach max_iter
together) and `clean` (every row noiseless: every codeword is valid at
iteration 0, so every step after a refill only hands out finished
codewords).  B = 2 * pool + 37 over pools of 64 and 192 lanes unless a case
says otherwise."""
import numpy as np
import pytest

from test_fused_rowblock_gpu import CHUNKS, LN49, MIXED_ITER, Case, _same

pytestmark = pytest.mark.gpu


class PathCase(Case):
    def noisy(self, B):
        if ("noisy", B) not in self._in:
            x = np.full((B, self.G.N), LN49)
            x[np.random.default_rng(78).random((B, self.G.N)) < 0.02] = -LN49
            x.setflags(write=False)
            self._in["noisy", B] = x
        return self._in["noisy", B]

    def clean(self, B):
        if ("clean", B) not in self._in:
            x = np.full((B, self.G.N), LN49)
            x.setflags(write=False)
            self._in["clean", B] = x
        return self._in["clean", B]

    def input(self, kind, B):
        return getattr(self, kind)(B)

    def oracle(self, kind, B, max_iter):
        k = (kind, B, max_iter)
        if k not in self._oracle:
            h, p, it, v = self.og.decode_batch(self.input(kind, B), max_iter, algo=0, post_mode=1, threads=16)
            assert not np.isnan(p).any()  # BP's guard: a NaN product is 1
            self._oracle[k] = (h, p, it, v.astype(bool))
        return self._oracle[k]


@pytest.fixture(scope="module")
def cases(gpu, oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_paths")
    made = {}

    def get(name):
        if name not in made:
            made[name] = PathCase(name, gpu, oracle_mod, tmp)
        return made[name]
    return get


def _on_off(c, kind, chunk, max_iter, sch, B=None):
    """Flag on and off: both equal the oracle and each other."""
    B = 2 * chunk + 37 if B is None else B
    x = c.input(kind, B)
    ref = c.oracle(kind, B, max_iter)
    out = {}
    for fuse in (True, False):
        s = dict(sch, resident=True, fuse_row_block=fuse)
        got = c.G.decode(x, max_iter=max_iter, post="ratio", chunk=chunk, schedule=s)
        _same(got, ref, (c.name, kind, chunk, B, max_iter, sch, fuse, "oracle"))
        out[fuse] = got
    _same(out[True], out[False], (c.name, kind, chunk, B, max_iter, sch, "on == off"))
    return out[True]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", ["reg4", "reg16"])
def test_lockstep_tiles(cases, name, chunk):
    """Every row noisy, max_iter 1, 2 and 5: a tile's lanes start together,
    run the plain path together and are `last` and `fresh` at once in the
    hand-over step (or, hand-over off, finished and refilled at once)."""
    c = cases(name)
    for mi in (1, 2, 5):
        for ho in (True, False):
            for table in (True, False):
                _, _, it, _ = _on_off(c, "noisy", chunk, mi, {"handover": ho, "lr_table": table})
                assert (it == mi).mean() > 0.5  # most lanes of a tile in lockstep to the end


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,chunk", [("reg4", 64), ("reg4", 192), ("reg16", 64), ("reg16", 192), ("rs7", 192)])
def test_mixed_tiles(cases, name, chunk):
    """Odd rows noiseless (lanes that finish at iteration 0 and are refilled
    while their neighbours are live: tiles on the path with all arms next to
    plain ones in one launch), coded and fp64 priors; and the Gaussian input
    with the directed NaN / huge / subnormal rows.
    Both kinds of step occurred: the codewords valid at iteration 0 are handed
    out and their lanes refilled beside live lanes, and once the input is
    used up (2 * pool + 37 codewords, half of them gone after one step each)
    the codewords that run on for ten and more iterations step without a
    refill, with steps in which none of a tile's lanes ends."""
    c = cases(name)
    for table in (True, False):
        for ho in (True, False):
            _, _, it, v = _on_off(c, "mixed", chunk, MIXED_ITER, {"handover": ho, "lr_table": table})
            assert (it[1::2] == 0).all() and v[1::2].all()
            assert it[0::2].max() >= 10
    for ho in (True, False):
        _, _, it, v = _on_off(c, "gauss", chunk, c.own_iter, {"handover": ho})
        assert len(np.unique(it)) > 3 and not v.all() and v.any() and it.max() >= 10


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_drain_finished_outputs_only(cases, chunk):
    """Tiles whose step holds finished codewords only (no live or refilled
    lane: no messages, no finisher).  `clean`: every codeword is valid at
    iteration 0, so each refill step is followed by such a step -- with one
    codeword, a ragged tile, and one codeword more than the pool (a whole
    pool of finished lanes beside one refilled lane, then the drain); and
    the mixed input's last tile."""
    c = cases("reg4")
    for B in (1, 37, chunk + 1):
        for ho in (True, False):
            for table in (True, False):
                _, _, it, v = _on_off(c, "clean", chunk, 5, {"handover": ho, "lr_table": table}, B=B)
                assert (it == 0).all() and v.all()
    _on_off(c, "mixed", chunk, 3, {"handover": False})


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_fp64_priors(cases, chunk):
    """The fp64-prior instantiation through decode: LLRs off the lattice,
    max_iter 1, 3 and the case's own."""
    c = cases("reg16")
    for mi in (1, 3, c.own_iter):
        for ho in (True, False):
            _on_off(c, "gauss", chunk, mi, {"handover": ho})


@pytest.mark.timeout(300)
def test_dna_code_once(gpu, cases):
    """The DNA code through its default 3-tile pool on coded lattice input,
    B = 2 * 192 + 37."""
    c = cases("dna")
    _, _, it, v = _on_off(c, "mixed", 192, 5, {"lr_table": True})
    assert (it[1::2] == 0).all() and v[1::2].all()
