"""Every configuration a GPU test hands the oracle (tests/oracle_configs.py), oracle against the real library (oracle/_ref): on the
edge-case corpus, on its 64-pair extract and on the batches of the test the configuration comes from, reduced to their smallest form —
status, score and op string, bit for bit.  The rows the library has no defined answer for (match < 0 with unequal or too short free begins,
DESIGN §5) are left out by one predicate, oracle_configs.reference_undefined, and never reach the library in this process: it reads cells it never wrote there and, depending on what
the heap held, faults.  tests/golden/oracle_grid.json records the library's results on the 64-pair extract (tools/make_oracle_grid_golden.py),
so that a configuration added to a GPU test without having been compared shows up, and the oracle is held to them where oracle/_ref is absent."""
import pytest

import common
import oracle_configs as oc
from oracle import loader

needs_ref = pytest.mark.skipif(not loader.have_reference(), reason="oracle/_ref not built (the real library's sources are not here)")

REG = oc.registry()
EXCLUDED = sorted(n for n, e in REG.items() if e["undefined"])
RUN = sorted(n for n, e in REG.items() if not e["undefined"] and not e["pinned_elsewhere"])
GOLDEN = common.load_golden("oracle_grid.json")["digests"]


special, digest, mini_config = oc.special, oc.digest, oc.mini_config


@needs_ref
@pytest.mark.parametrize("name", RUN)
def test_oracle_equals_reference(name):
    e = REG[name]
    sp, mini = special()
    batches = [("special", sp), ("special_mini", mini)] + [(repr(s), oc.batch_of(s, e["kw"])) for s in e["shapes"]]
    # at least one batch of the row's own has room for its free ends as written (on the edge-case corpora they clamp to 0)
    assert any(common.clamp_free(e["kw"], batch) == e["kw"] for _, batch in batches[2:]), (name, "no batch keeps the free ends intact")
    for label, batch in batches:
        kw = common.clamp_free(e["kw"], batch)
        assert not oc.reference_refuses(kw), (name, label, "the library exits on this configuration")
        assert not oc.reference_undefined(kw), (name, label, "clamping the free ends made the row one the reference has no answer for")
        cfg = loader.make_config(**kw)
        loader.oracle_undefined_reads(True)
        o = loader.run(loader.oracle(), cfg, batch)
        # (the oracle counts its reads of the reference's unwritten offsets[0]: the registry's predicate must have kept every such row
        # out — nothing is skipped here, and nothing undefined reaches the library)
        assert loader.oracle_undefined_reads() == 0, (name, label, "oracle_configs.reference_undefined misses this row")
        r = loader.run(loader.reference(), cfg, batch)
        common.assert_same(r, o["score"], o["status"], o["cigars"], batch, f"oracle vs reference {kw} on {label} ({e['sources'][0]})")
        if label == "special_mini":
            assert digest(r) == GOLDEN.get(name), (name, "tests/golden/oracle_grid.json is stale: tools/make_oracle_grid_golden.py")


def test_excluded_rows_are_exactly_the_undefined_ones():
    """Nothing is left out but by the predicate, and the predicate may not grow into a way round the comparison: at most 5 % of the rows."""
    left_out = sorted(set(REG) - set(RUN) - {n for n, e in REG.items() if e["pinned_elsewhere"]})
    assert left_out == EXCLUDED == sorted(n for n, e in REG.items() if oc.reference_undefined(e["kw"]))
    assert not any(oc.reference_undefined(REG[n]["kw"]) for n in RUN)
    assert all(REG[n]["kw"].get("match", 0) < 0 for n in EXCLUDED)
    assert len(EXCLUDED) <= 0.05 * len(REG), (len(EXCLUDED), len(REG))
    # the two rows of the parity grid (GRID[93] and GRID[94]) are among them
    assert sum(1 for n in EXCLUDED if any(s.startswith("test_parity_gpu.GRID[") for s in REG[n]["sources"])) == 2


def test_biwfa_rows_marked_as_pinned_elsewhere_are():
    pinned = [e for e in REG.values() if e["pinned_elsewhere"]]
    assert pinned and all(e["biwfa"] and e["key"] in oc.already_pinned() for e in pinned)


def test_registry_covers_the_gpu_tests_configuration_lists():
    """Every configuration list of the GPU test modules is collected (or waived with a reason), every row of a collected list is in the
    registry under the fields `loader.make_config` gives it, and every row that is defined has the library's recorded result: a row added
    to tests/test_parity_gpu.py GRID fails here until it has been run against the library (tools/make_oracle_grid_golden.py)."""
    for module in oc.MODULES:
        for name, obj in oc.config_lists(module):
            assert oc.is_declared(obj), f"{module}.{name} holds configurations but is neither in oracle_configs.SOURCES nor in WAIVED"
    for reason in oc.WAIVED.values():
        assert reason
    by_key = {e["key"]: e for e in REG.values()}
    missing = []
    for module, attr, expand, _ in oc.SOURCES:
        rows = oc.rows_of(module, attr)
        assert rows, (module, attr)
        for i, row in enumerate(rows):
            for kw in expand(i, row):
                e = by_key.get(oc.key_of(kw))
                assert e is not None and f"{module}.{attr}[{i}]" in e["sources"], (module, attr, i)
                if not e["undefined"] and e["name"] not in GOLDEN:
                    missing.append(f"{module}.{attr}[{i}] {e['name']}")
    assert not missing, f"not compared with the library yet (tools/make_oracle_grid_golden.py): {missing}"
    assert sorted(GOLDEN) == sorted(n for n, e in REG.items() if not e["undefined"])
    assert not [n for n, e in REG.items() if oc.reference_refuses(e["kw"])]


def test_configurations_written_inside_test_functions_match_a_registry_entry():
    """What the walk over module-level lists cannot see: every `dict(...)` / `configs_pair(...)` / `make_config(...)` literal in the source
    of the GPU test modules agrees, on the fields it names, with some registry entry — the registry gives a literal that matches no
    collected row an entry of its own, and test_registry_covers_... wants the library's recorded result for it: a step limit, a penalty
    shape or free ends written into a test function fail there until compared.  (Weaker than the walk over lists: the fields a literal
    leaves open, such as a scope or a step limit taken from a variable, are not checked.)"""
    loose = []
    for module in oc.MODULES + oc.SCANNED_ONLY:
        for line, kw in oc.literal_configs(module):
            if (module, tuple(sorted(kw.items()))) not in oc.WAIVED_LITERALS and not oc.matches_an_entry(kw):
                loose.append(f"{module}:{line} {kw}")
    assert not loose, loose
    for reason in oc.WAIVED_LITERALS.values():
        assert reason


def test_oracle_reproduces_the_recorded_reference_results():
    """Without oracle/_ref: the oracle's results on the 64 edge-case pairs are the ones the library gave when the row was recorded."""
    bad = []
    for name, e in REG.items():
        if e["undefined"]:
            continue
        cfg, mini = mini_config(e)
        if digest(loader.run(loader.oracle(), cfg, mini)) != GOLDEN.get(name):
            bad.append(name)
    assert not bad, bad
