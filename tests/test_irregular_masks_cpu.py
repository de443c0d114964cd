"""CPU suite: the irregular-mask generator (trajsde_amd/synth.py irregular_masks) and what its batches can see.

synth() makes a padded prefix followed by one valid run (or one pattern for every row) and always observes step 20.  On such
inputs every masked GRU step comes after the iteration whose state the encoder keeps, "first bos" and "last bos" are one index,
and no agent loses its global edges -- so three mis-statements of the mask handling leave every output unchanged.  The second
half of this file applies them to the float64 oracle and shows that the irregular batch of helpers.TRAINED_CASES moves by far
more than the GPU tests' bound, while the old prefix-padded case does not move at all."""
import pytest
import torch

import helpers as H
from trajsde_amd.synth import (CAT_FULL, CAT_GONE_AT_20, CAT_NEVER, CAT_ONLY_20, CAT_RUNS, CATEGORY_NAMES, T_HIST, irregular,
                               irregular_masks, mask_categories, synth)


def _counts(batch):
    return torch.bincount(mask_categories(batch), minlength=5).tolist()


@pytest.mark.parametrize("name", H.IRREGULAR_CASES)
def test_irregular_cases_hold_every_row_kind(name):
    """the trained-weight batches: every kind at least twice (printed: the count per kind), agents observed at step 20 with a gap,
    some first bos after step 0, rows observed at step 20 without a valid future step, kinds adjacent within a 16-row tile"""
    K, T, max_t, make = H.TRAINED_CASES[name]
    b = make()
    cat, pm, bos, ag = mask_categories(b), b["padding_mask"], b["bos_mask"], b["agent_index"]
    counts = _counts(b)
    no_future = ~pm[:, T_HIST - 1] & pm[:, T_HIST:].all(1)
    print(f"[irregular] {name}: N={b.num_nodes} A={ag.numel()} " + ", ".join(f"{n} {c}" for n, c in zip(CATEGORY_NAMES, counts)) +
          f", observed at 20 without a valid future {int(no_future.sum())}")
    assert int(cat.min()) >= 0 and min(counts) >= 2
    assert int(no_future.sum()) >= 2
    assert not bool(pm[ag, T_HIST - 1].any()) and bool((bos[ag].sum(1) >= 2).all()) and bool((~bos[ag, 0]).any())
    valid = ~pm[ag, :T_HIST]
    for v in valid:                                                          # an interior gap: padded steps between two valid ones
        first, last = int(torch.nonzero(v)[0]), int(torch.nonzero(v)[-1])
        assert last == T_HIST - 1 and not bool(v[first:last].all())
    for tile in range(0, b.num_nodes - 15, 16):                              # a whole tile never holds one kind only
        assert len(set(cat[tile:tile + 16].tolist())) >= 4
    if name == "irregular_k6_t20":
        assert (b.num_nodes + ag.numel()) % 16 != 0
    else:                                                                    # period 5 against tiles of 16: every offset occurs
        for c in range(5):
            assert {int(i) % 16 for i in torch.nonzero(torch.arange(b.num_nodes) % 5 == c)[:, 0]} == set(range(16))


def test_irregular_masks_follow_the_preprocessing_rules():
    plain = synth(S=3, n=13, L=5, F=12, box=80.0, seed=31, mixed_source=True)
    b = irregular(S=3, n=13, L=5, F=12, box=80.0, seed=31, mixed_source=True)
    again = irregular_masks(synth(S=3, n=13, L=5, F=12, box=80.0, seed=31, mixed_source=True), 31, 12)
    other = irregular_masks(synth(S=3, n=13, L=5, F=12, box=80.0, seed=31, mixed_source=True), 32, 12)
    for k in ("padding_mask", "bos_mask", "x"):
        assert torch.equal(b[k], again[k]), k                                # one seeded generator
    assert not torch.equal(b["padding_mask"], other["padding_mask"])
    for k in b.keys:                                                         # nothing else is touched
        if k not in ("padding_mask", "bos_mask", "x") and torch.is_tensor(b[k]):
            assert torch.equal(b[k], plain[k]), k
    pm, bos, x, pos = b["padding_mask"], b["bos_mask"], b["x"], b["positions"]
    valid = ~pm[:, :T_HIST]
    assert torch.equal(bos[:, 0], valid[:, 0]) and torch.equal(bos[:, 1:], valid[:, 1:] & ~valid[:, :-1])
    both = valid[:, 1:] & valid[:, :-1]
    disp = pos[:, 1:T_HIST] - pos[:, :T_HIST - 1]
    assert torch.equal(x[:, 1:][both], disp[both]) and not bool(x[:, 1:][~both].any()) and not bool(x[:, 0].any())
    assert bool(pm[pm[:, T_HIST - 1]][:, T_HIST:].all())                     # unobserved at step 20: no future (the reference's rule)
    cat = mask_categories(b)
    rest = ~torch.isin(torch.arange(39), b["agent_index"])
    assert torch.equal(cat[rest], (torch.arange(39) % 5)[rest])              # round-robin over the node index
    assert bool((cat[b["agent_index"]] == CAT_RUNS).all())
    assert {CAT_FULL, CAT_RUNS, CAT_GONE_AT_20, CAT_NEVER, CAT_ONLY_20} == set(cat.tolist())


def test_irregular_masks_refuse_a_batch_without_the_hard_rows():
    with pytest.raises(AssertionError):
        irregular_masks(synth(S=1, n=6, L=3, F=5, box=40.0, seed=1), 1, 5)    # 6 rows: one of each kind at the most


# ----------------------------------------------------------------------------- the mis-statements
NAME, OLD = "irregular_k6_t20", "argo_dropout_k6_t30"
SEED = 6


def _case(name):
    from trajsde_amd.models.model_base_mix_sde import PredictionModelSDENet
    K, T, max_t, make = H.TRAINED_CASES[name]
    cfg = H.our_cfg(K, T, max_t)
    model = PredictionModelSDENet(**cfg, init_seed=2).eval()
    H.trained_like_parameters(model, H.TRAINED_SEED, 1.0)
    return model, cfg, make()


_CASES = {}


def _loc(name):
    """(loc of the float64 oracle as it stands -- computed once --, a function that computes it again)"""
    if name not in _CASES:
        model, cfg, batch = _case(name)
        run = lambda: H.oracle_forward64(model, cfg, batch, noise_seed=SEED, want_intermediates=False)["loc"]   # noqa: E731
        _CASES[name] = (run(), run)
    return _CASES[name]


def _last_bos(monkeypatch):
    """(a) the kept iteration from the LAST bos of a row, not the first"""
    stock = torch.argmax

    def argmax(t, dim=None, **kw):
        if dim == 1 and t.dim() == 2 and t.shape[1] == T_HIST:               # eos = ref_time - argmax(bos_mask) (ENC:187)
            return t.shape[1] - 1 - stock(t.flip(1), dim=1)
        return stock(t, dim=dim, **kw)
    monkeypatch.setattr(torch, "argmax", argmax)


def _masked_step_keeps_the_pre_sde_state(monkeypatch):
    """(b) a masked GRU step hands on the state from before the SDE step, not h_ode"""
    import restate
    stock, state = restate.gru_unit, {"calls": 0}

    def gru_unit(P, pre, h_cur, x, mask):
        before = P["encoder.hidden"].unsqueeze(0).expand_as(h_cur) if state["calls"] % T_HIST == 0 else state["h"]
        state["calls"] += 1
        state["h"] = torch.where(mask.unsqueeze(-1), stock(P, pre, h_cur, x, mask), before)
        return state["h"]
    monkeypatch.setattr(restate, "gru_unit", gru_unit)


def _validity_of_the_row_above(monkeypatch):
    """(b'), the sibling: whether a row's step is masked is read from the row above (a `valid` picked from the wrong row of a tile)"""
    import restate
    stock = restate.gru_unit
    monkeypatch.setattr(restate, "gru_unit", lambda P, pre, h_cur, x, mask: stock(P, pre, h_cur, x, torch.roll(mask, 1, 0)))


def _padded_agents_keep_their_global_edges(monkeypatch):
    """(c) the global interactor does not drop the edges of the agents padded at step 20"""
    import restate
    stock = restate.global_interactor

    def global_interactor(P, cfg, batch, *a, **kw):
        b = H.clone_batch(batch)
        b["padding_mask"][:, cfg["historical_steps"] - 1] = False
        return stock(P, cfg, b, *a, **kw)
    monkeypatch.setattr(restate, "global_interactor", global_interactor)


MUTATIONS = {"last_bos": _last_bos, "pre_sde_state": _masked_step_keeps_the_pre_sde_state,
             "row_above": _validity_of_the_row_above, "padded_agents_keep_edges": _padded_agents_keep_their_global_edges}


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_irregular_batch_sees_the_mis_statement(mutation, monkeypatch):
    """each mis-statement moves loc by more than 100 x the GPU tests' bound, on their own scaled measure"""
    from test_gpu_trained_weights import TOL, _scaled
    want, run = _loc(NAME)
    MUTATIONS[mutation](monkeypatch)
    moved = _scaled(run(), want)
    print(f"[irregular] {mutation} moves loc of {NAME} by {moved:.2e} (scaled); the bound is {TOL:.0e}")
    assert moved > 100 * TOL


@pytest.mark.parametrize("mutation", ["last_bos", "pre_sde_state"])
def test_prefix_padded_batch_cannot_see_the_mis_statement(mutation, monkeypatch):
    """why the earlier inputs never exercised these lines: one bos per row, and every masked step after the kept iteration"""
    want, run = _loc(OLD)
    assert bool(H.TRAINED_CASES[OLD][3]()["padding_mask"][:, :T_HIST].any())   # it does have padded steps
    MUTATIONS[mutation](monkeypatch)
    assert torch.equal(run(), want)


def test_uniform_sparsity_cannot_see_a_validity_taken_from_another_row(monkeypatch):
    """... and why the every-fifth-step pattern does not exercise (b'): all rows share one mask"""
    batch, meta, out, mid = H.load_fixture("nus_k1_t5")
    model, cfg = H.build_model(meta)
    want = H.oracle_forward(model, cfg, batch, meta["noise_seed"], want_intermediates=False)["loc"]
    _validity_of_the_row_above(monkeypatch)
    assert torch.equal(H.oracle_forward(model, cfg, batch, meta["noise_seed"], want_intermediates=False)["loc"], want)
