"""GPU suite (-m gpu): the Neumann-Neumann induced and the LORASC preconditioner on the synthetic partitioned systems of
tests/full_synth.py, at the shapes box and pie partitions of small meshes never produce (the inputs' properties and the
restatements' own noise are asserted on the host by tests/test_full_synth_cpu.py).

  (a) the induced apply on `tiles` and `panels` under all nine RPW x WAVES tilings of k_gemv_nni, both storages, both
      couplings: 1e-10 against the refined restatement (DESIGN §3's bar for the device's exact elimination against the host;
      fp32 against the restatement on the rounded blocks), and every tiling bit-identical to the first one that ran — the
      as-written coupling carries z_loc into the interior part, the assembled one the slots;
  (b) r_I = 0: z[pos_Γ] carries the bits of `NeumannNeumannSchurPreconditioner.ldiv(r_Γ)` created under the same tiling;
  (c) slot widths 1, 4 (3 widened) and 6, a Γ node without interior coupling, a subdomain without interior: both operators,
      index base 1, repeated applies and device pointers bit-identical;
  (d) LORASC's partial dots: n_Γ = 768 + r over four workgroups with nev = 0 ... 1024, `set_correction` down and up again
      against fresh creates, the refusal of 1025;
  (e) `pcg` / `defpcg` on the consistent `solve` system against the oracle with the dense restated M^-1, under three tilings,
      eager against replayed.
Every 1e-10 comparison prints its error and margin; measured figures: DESIGN §3."""
import numpy as np
import pytest

from conftest import lowest_eigvecs
from test_gpu_lorasc import _assert_solve
import full_synth as fs
import lorasc_ref as lr
import nn_induced_ref as nr

pytestmark = pytest.mark.gpu

APPLY_BAR = 1e-10
STORAGES = ("f64", "f32")
DEFAULT_CHUNK = 8
_FIRST, _WANT, _COUNT = {}, {}, {"bitwise": 0, "worst": {}}


def same_bits(a, b, what):
    _COUNT["bitwise"] += 1
    assert np.array_equal(a, b), f"{what}: {np.count_nonzero(a != b)} of {a.size} entries differ, max |Δ| {np.max(np.abs(a - b)):.3e}"


def within_bar(got, want, group, what):
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    _COUNT["worst"][group] = max(_COUNT["worst"].get(group, 0.0), err)
    print(f"{what}: rel. error {err:.3e} (bar {APPLY_BAR:.0e}, margin {APPLY_BAR / max(err, 1e-300):.1f}x)")
    assert err <= APPLY_BAR, (what, err)


@pytest.fixture(scope="module", autouse=True)
def tally():
    yield
    print(f"\nfull_synth edges: {_COUNT['bitwise']} bitwise comparisons; worst rel. error per group: "
          + ", ".join(f"{k} {v:.2e}" for k, v in sorted(_COUNT["worst"].items())))
    _FIRST.clear()
    _WANT.clear()
    fs.drop()


@pytest.fixture(scope="module")
def setups(pkg, ctx):
    """one set-up plan with kept levels per case, built when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            P = fs.case(name).P
            s = pkg.api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
            s.keep_levels()
            s.run()
            made[name] = s
        return made[name]
    yield get
    for s in made.values():
        s.close()


def set_tiling(monkeypatch, rpw, waves):
    monkeypatch.setenv("MI355_GEMV_RPW", str(rpw))
    monkeypatch.setenv("MI355_GEMV_WAVES", str(waves))


def blocks_for(fem, c, storage):
    ΠSd = nr.prepare(fem, c)
    return nr.rounded_f32(ΠSd) if storage == "f32" else ΠSd


def induced(pkg, ctx, fem, c, setup, storage="f64", coupling="reference", index_base=0):
    sub = c.P.sub
    return pkg.api.NeumannNeumannInducedPreconditioner(ctx, c.P.A_IΓdd, (c.pos_I, c.pos_Γ), sub.gather_idx, sub.node_Γ_cnt,
                                                      nr.prepare(fem, c), setup, storage=storage, coupling=coupling,
                                                      index_base=index_base)


def induced_want(fem, c, storage, cpl, r, tag="r"):
    key = (c.name, storage, cpl, tag)
    if key not in _WANT:
        _WANT[key] = nr.apply_neumann_neumann_induced(c, blocks_for(fem, c, storage), r, cpl, refine=2)
    return _WANT[key]


# ------------------------------------------------------------------ (a) the induced apply at every tiling
@pytest.mark.parametrize("waves", fs.WAVES)
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", ["tiles", "panels"])
def test_induced_apply_every_tiling(pkg, ctx, fem, setups, monkeypatch, name, storage, waves):
    """The tiling decides only which wave owns a row of ΠS_d (GemvRows, as in k_gemv_batched): all nine must give the same
    bits in the slots and in z_loc. RPW = 1 of every WAVES is held to the restatement; every tiling to the first that ran."""
    c = fs.case(name)
    r = nr.apply_input(c)
    for rpw in fs.RPWS:
        set_tiling(monkeypatch, rpw, waves)
        M = induced(pkg, ctx, fem, c, setups(name), storage)
        try:
            for cpl in nr.COUPLINGS:
                M.set_coupling(cpl)
                z = M.ldiv(r)
                tag = f"induced apply {name} {storage} {cpl} {rpw} x {waves}"
                if rpw == fs.RPWS[0]:
                    within_bar(z, induced_want(fem, c, storage, cpl, r), f"(a) {name}", tag)
                same_bits(z, _FIRST.setdefault((name, storage, cpl), z), tag + " against the first tiling")
        finally:
            M.close()


# ------------------------------------------------------------------ (b) the Neumann-Neumann stage, bit for bit
@pytest.mark.parametrize("waves", fs.WAVES)
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", ["tiles", "panels", "w1", "w3", "hub6"])
def test_nn_stage_bits_every_tiling(pkg, ctx, fem, setups, monkeypatch, name, storage, waves):
    """r_I = 0: every column sum is +0 and r_schur = r_Γ exactly, so z[pos_Γ] is the existing Neumann-Neumann operator's
    ldiv(r_Γ) on the same ΠS_d, storage and tiling; the whole z matches the restatement in the same run"""
    api = pkg.api
    c = fs.case(name)
    sub = c.P.sub
    r = np.zeros(c.n)
    r[c.pos_Γ] = np.random.default_rng(9).standard_normal(c.n_Γ)
    for rpw in fs.RPWS:
        set_tiling(monkeypatch, rpw, waves)
        Πnn = api.NeumannNeumannSchurPreconditioner(ctx, nr.prepare(fem, c), sub.gather_idx, sub.node_Γ_cnt, storage=storage)
        want_Γ = Πnn.ldiv(r[c.pos_Γ])
        Πnn.close()
        M = induced(pkg, ctx, fem, c, setups(name), storage)
        try:
            for cpl in nr.COUPLINGS:
                M.set_coupling(cpl)
                z = M.ldiv(r)
                tag = f"nn stage {name} {storage} {cpl} {rpw} x {waves}"
                same_bits(z[c.pos_Γ], want_Γ, tag)
                if rpw == fs.RPWS[-1]:
                    within_bar(z, induced_want(fem, c, storage, cpl, r, "r_I = 0"), f"(b) {name}", tag)
        finally:
            M.close()


# ------------------------------------------------------------------ (c) widths, bare nodes, empty interior
@pytest.mark.parametrize("name", fs.WIDTH_CASES)
def test_induced_widths_bare_and_empty(pkg, ctx, fem, setups, name):
    """k_nni_assemble at slot widths 1, 4 and 6; `bare`: a Γ node whose gseg range is empty (z = r[pos] untouched) and a
    subdomain with n_i = 0 (pos_I NULL, no entries)"""
    import torch
    c = fs.case(name)
    r = nr.apply_input(c)
    for storage in STORAGES:
        M = induced(pkg, ctx, fem, c, setups(name), storage)
        M1 = induced(pkg, ctx, fem, c, setups(name), storage, index_base=1)
        for cpl in nr.COUPLINGS:
            M.set_coupling(cpl)
            M1.set_coupling(cpl)
            z = M.ldiv(r)
            tag = f"induced {name} {storage} {cpl}"
            within_bar(z, induced_want(fem, c, storage, cpl, r), f"(c) induced {name}", tag)
            same_bits(M.ldiv(r), z, tag + " second apply")
            same_bits(M1.ldiv(r), z, tag + " index base 1")
            same_bits(pkg.api.apply_neumann_neumann_induced(M, torch.from_numpy(r).cuda()).cpu().numpy(), z, tag + " device pointers")
        M.close()
        M1.close()


def lorasc(pkg, ctx, c, setup, E=None, coef=None, index_base=0):
    gg = pkg.api.SparseDirectPreconditioner(ctx, c.A_ΓΓ)
    return pkg.api.LorascPreconditioner(ctx, c.A_IΓd, (c.pos_I, c.pos_Γ), setup, gg, E, coef, index_base=index_base)


@pytest.mark.parametrize("name", fs.WIDTH_CASES)
def test_lorasc_widths_bare_and_empty(pkg, ctx, setups, name):
    """the column form of k_lo_zgamma with 1 ... 6 segments per node and none; nev = 0 and 5"""
    import torch
    c = fs.case(name)
    for nev, with_coef in ((0, False), (5, False), (5, True)):
        x, E, coef = lr.apply_inputs(c, nev, with_coef)
        M = lorasc(pkg, ctx, c, setups(name), E, coef)
        M1 = lorasc(pkg, ctx, c, setups(name), E, coef, index_base=1)
        z = M.ldiv(x)
        tag = f"lorasc {name} nev {nev} coef {'random' if with_coef else 'NULL'}"
        within_bar(z, lr.apply_lorasc(c, x, E, coef, refine=2), f"(c) lorasc {name}", tag)
        same_bits(M.ldiv(x), z, tag + " second apply")
        same_bits(M1.ldiv(x), z, tag + " index base 1")
        same_bits(pkg.api.apply_lorasc(M, torch.from_numpy(x).cuda()).cpu().numpy(), z, tag + " device pointers")
        M.close()
        M1.close()


# ------------------------------------------------------------------ (d) LORASC's partial dots
@pytest.mark.parametrize("name", fs.WG_CASES)
def test_lorasc_partial_dots(pkg, ctx, setups, name):
    """n_Γ = 768 + r: four workgroups, the last one's strided terms cut at every position; nev = 1 ... 5 (waves of
    k_lo_zgamma idle, one pass, one pass and one more), 255 / 256 / 257 (the 256-thread loop of k_lo_correct) and 1024 (the LDS
    table full), coef NULL and random"""
    c = fs.case(name)
    M = lorasc(pkg, ctx, c, setups(name))
    for nev in fs.NEV_ALL:
        for with_coef in ((False, True) if nev else (False,)):
            x, E, coef = lr.apply_inputs(c, nev, with_coef)
            M.set_correction(E, coef)
            z = M.ldiv(x)
            within_bar(z, lr.apply_lorasc(c, x, E, coef, refine=2), f"(d) {name}",
                       f"lorasc {name}: n_Γ = {c.n_Γ}, nev = {nev}, coef = {'random' if with_coef else 'NULL'}")
    M.close()


@pytest.mark.parametrize("name", ["wg1", "wg193"])
def test_lorasc_correction_shrinks_and_regrows(pkg, ctx, setups, name):
    """set_correction from 1024 vectors down to 3 and back up equals fresh creates, bit for bit (E, coef and the partials
    shrink and regrow in place); nev = 1025 is MI_ERR_BAD_ARG with a message from create and from set_correction, and the
    operator applies to the same bits afterwards"""
    api, L = pkg.api, pkg._lib
    c = fs.case(name)
    x, E_big, coef_big = lr.apply_inputs(c, fs.LO_MAX_NEV, True)
    _, E_small, coef_small = lr.apply_inputs(c, 3, True)
    fresh_big = lorasc(pkg, ctx, c, setups(name), E_big, coef_big)
    fresh_small = lorasc(pkg, ctx, c, setups(name), E_small, coef_small)
    z_big, z_small = fresh_big.ldiv(x), fresh_small.ldiv(x)
    fresh_small.close()
    assert not np.array_equal(z_big, z_small)
    within_bar(z_big, lr.apply_lorasc(c, x, E_big, coef_big, refine=2), f"(d) {name}", f"lorasc {name} nev 1024")
    M = fresh_big
    for k, (E, coef, want) in enumerate(((E_small, coef_small, z_small), (E_big, coef_big, z_big), (None, None, None),
                                         (E_big, coef_big, z_big), (E_small, coef_small, z_small))):
        M.set_correction(E, coef)
        if want is not None:
            same_bits(M.ldiv(x), want, f"lorasc {name} set_correction step {k}")
    M.set_correction(E_big, coef_big)
    too_many = np.zeros((c.n_Γ, fs.LO_MAX_NEV + 1))
    with pytest.raises(api.MiError) as e:
        M.set_correction(too_many)
    assert e.value.code == L.MI_ERR_BAD_ARG and "1025" in str(e.value) and "1024" in str(e.value) and len(str(e.value)) > 40
    with pytest.raises(api.MiError) as e:
        lorasc(pkg, ctx, c, setups(name), too_many)
    assert e.value.code == L.MI_ERR_BAD_ARG and "1025" in str(e.value) and "1024" in str(e.value) and len(str(e.value)) > 40
    same_bits(M.ldiv(x), z_big, f"lorasc {name} after the refused 1025")
    M.close()


# ------------------------------------------------------------------ (e) one solve
@pytest.fixture(scope="module")
def solve_refs(fem, orc):
    c = fs.case("solve")
    Ao = orc.csc_operator(c.A)
    ϕ = lowest_eigvecs(Ao, c.n, c.P.sub.ndom + 10)
    x0 = np.zeros(c.n)
    out = {"Ao": Ao, "ϕ": ϕ}
    for storage in STORAGES:
        Minv = nr.dense_minv(c, blocks_for(fem, c, storage), "assembled")
        Mo = orc.neumann_neumann_operator([Minv], [np.arange(c.n)], np.ones(c.n, dtype=np.int64))
        out[storage] = (orc.pcg(Ao, c.b, x0, Mo, 0, fs.EPS), orc.defpcg(Ao, c.b, x0, ϕ, Mo, 0, fs.EPS))
    return out


@pytest.mark.parametrize("storage,rpw,waves", [("f64", 2, 16), ("f64", 1, 4), ("f32", 4, 8)], ids=["default", "f64-1x4", "f32-4x8"])
def test_solve_against_oracle(pkg, ctx, fem, setups, solve_refs, monkeypatch, storage, rpw, waves):
    """pcg(A, b, 0, M) and defpcg(A, b, 0, ϕ, M) with the assembled coupling against the oracle with the dense restated M^-1
    (on the rounded blocks for fp32: `it` equal); eager == replayed in chunks of 4, bit for bit: the launches after the stop
    return on `done` in every kernel of the apply"""
    api = pkg.api
    c = fs.case("solve")
    if (rpw, waves) == (2, 16):
        monkeypatch.delenv("MI355_GEMV_RPW", raising=False)
        monkeypatch.delenv("MI355_GEMV_WAVES", raising=False)
    else:
        set_tiling(monkeypatch, rpw, waves)
    A = api.SparseMatrixCSC(ctx, c.A)
    M = induced(pkg, ctx, fem, c, setups("solve"), storage, "assembled")
    x0, ϕ, Ao = np.zeros(c.n), solve_refs["ϕ"], solve_refs["Ao"]
    want_pcg, want_def = solve_refs[storage]
    runs = {}
    try:
        for chunk in (DEFAULT_CHUNK, 0, 4):
            ctx.set_chunk(chunk)
            runs[chunk] = (api.pcg(A, c.b, x0, M, 0, fs.EPS), api.defpcg(A, c.b, x0, ϕ, M, 0, fs.EPS))
    finally:
        ctx.set_chunk(DEFAULT_CHUNK)
    for got, want, kind in zip(runs[DEFAULT_CHUNK], (want_pcg, want_def), ("pcg", "defpcg")):
        print(f"solve {kind} {storage} {rpw} x {waves}: ", end="")
        if storage == "f64":
            _assert_solve(got, want, Ao, c.b)
        else:
            print(f"it = {got[1]} (oracle {want[1]}), max rel. history difference {np.max(np.abs(got[2] - want[2][:len(got[2])]) / want[2][:len(got[2])]):.3e}")
        assert got[1] == want[1] and got[1] <= 50
    for k, kind in enumerate(("pcg", "defpcg")):
        eager, replay = runs[0][k], runs[4][k]
        assert eager[1] == replay[1] == runs[DEFAULT_CHUNK][k][1]
        same_bits(replay[0], eager[0], f"solve {kind} {storage} {rpw} x {waves}: x, replayed against eager")
        same_bits(replay[2], eager[2], f"solve {kind} {storage} {rpw} x {waves}: res_norm, replayed against eager")
        same_bits(runs[DEFAULT_CHUNK][k][0], eager[0], f"solve {kind} {storage} {rpw} x {waves}: x, default chunk against eager")
    M.close()
    A.close()
