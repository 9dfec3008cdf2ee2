"""The analysis options' record and its table of rules (mgatk2_amd/options.py): every rule of
REQUIRES is refused by the command line, by MtDNAPipeline and by CellProcessor.enable, and every
range checker refuses its edges and takes its boundaries. No device."""

import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from mgatk2_amd.exceptions import InvalidInputError
from mgatk2_amd.options import FLAGS, REQUIRES, AnalysisOptions

ROOT = Path(__file__).resolve().parent.parent
VALUES = {"call_variants": True, "cluster": True, "clones": 3, "neighbors": 10, "snn_prune": 0.5, "clonotypes": True,
          "clonotype_resolution": 2.0}
# the stage an option turns on or belongs to (call_variants: enable_variants)
STAGE_OF = {"cluster": "cluster", "clones": "cluster", "neighbors": "neighbors", "snn_prune": "neighbors",
            "clonotypes": "clonotypes", "clonotype_resolution": "clonotypes"}
RULES = [pytest.param(o, n, id=f"{o}-needs-{n}") for o, n in REQUIRES]


def breaking(option, needs):
    """Keywords that break one rule only: `option`, and all that `needs` needs, without `needs`."""
    kw, todo = {option: VALUES[option]}, [needs]
    while todo:
        for o, n in REQUIRES:
            if o == todo[0] and n not in kw:
                kw[n] = VALUES[n]
                todo.append(n)
        todo.pop(0)
    assert needs not in kw
    return kw


def test_the_table_covers_the_record():
    names = list(AnalysisOptions.__dataclass_fields__)
    assert names == list(FLAGS) == list(VALUES) and len(names) == 7
    assert {o for o, _ in REQUIRES} == set(names) - {"call_variants"}  # every option but the first needs another
    assert AnalysisOptions().given() == {}
    AnalysisOptions().check(InvalidInputError)
    AnalysisOptions(**VALUES).check(InvalidInputError)
    assert AnalysisOptions(**VALUES).given() == VALUES
    # 0 and 0.0 are values, not "not given"
    assert AnalysisOptions(True, neighbors=5, snn_prune=0.0).given() == dict(call_variants=True, neighbors=5,
                                                                           snn_prune=0.0)
    with pytest.raises(AttributeError):
        AnalysisOptions().cluster = True


@pytest.mark.parametrize("option, needs", RULES)
def test_rule_refused_by_the_cli(option, needs, tmp_path, monkeypatch):
    from click.testing import CliRunner

    from mgatk2_amd import cli as cli_mod
    from mgatk2_amd import pipeline

    seen = []
    monkeypatch.setattr(pipeline, "run_pipeline", lambda **kw: seen.append(kw) or {})
    args = []
    for name, v in breaking(option, needs).items():
        args += [FLAGS[name]] if v is True else [FLAGS[name], str(v)]
    for cmd in ("run", "tenx", "call"):
        r = CliRunner().invoke(cli_mod.cli, [cmd, "-i", str(tmp_path), "-o", str(tmp_path / "out"), *args])
        assert r.exit_code == 2 and f"{FLAGS[option]} requires {FLAGS[needs]}" in r.output, (cmd, r.output)
    assert seen == []
    with pytest.raises(cli_mod.click.UsageError, match=f"^{FLAGS[option]} requires {FLAGS[needs]}$"):
        AnalysisOptions(**breaking(option, needs)).check(cli_mod.click.UsageError)


@pytest.mark.parametrize("option, needs", RULES)
def test_rule_refused_by_the_pipeline(option, needs, tmp_path):
    from mgatk2_amd.pipeline import MtDNAPipeline

    kw = breaking(option, needs)
    if option == "snn_prune":
        # the keyword's default is a float, so the pipeline cannot see it given: taken without
        # neighbors (and unused), as it always was; the options pass and the BAM is looked for
        with pytest.raises(InvalidInputError, match="BAM file not found"):
            MtDNAPipeline("no.bam", ["A"], tmp_path, **kw)
        return
    text = f"{option} needs {needs} ({FLAGS[option]} requires {FLAGS[needs]})"
    with pytest.raises(InvalidInputError) as e:
        MtDNAPipeline("no.bam", ["A"], tmp_path, **kw)  # (refused before the BAM, which is not there, is opened)
    assert str(e.value) == text
    with pytest.raises(InvalidInputError, match="BAM file not found"):
        MtDNAPipeline("no.bam", ["A"], tmp_path, **kw, **{needs: VALUES[needs]})


@pytest.mark.parametrize("option, needs", RULES)
def test_rule_refused_by_the_processor(option, needs, tmp_path):
    from mgatk2_amd.analysis.stages import STAGES
    from mgatk2_amd.processing.processors import CellProcessor

    assert list(STAGES) == [s.key for s in STAGES.values()] == ["cluster", "neighbors", "clonotypes"]
    stage = STAGES[STAGE_OF[option]]
    if STAGE_OF.get(needs) == stage.key:
        # an option of the stage that it needs: given to that stage's enable and nowhere else
        name = {"clones": "clones", "snn_prune": "prune", "clonotype_resolution": "resolution"}[option]
        assert name in [n for n, _, _ in stage.options]
        assert all(name not in [n for n, _, _ in s.options] for s in STAGES.values() if s is not stage)
        return
    assert stage.needs == STAGE_OF.get(needs, "variants")
    proc = CellProcessor(None, tmp_path)
    for name in reversed(list(breaking(option, needs))[1:]):  # what `needs` needs, the first needed last
        proc.enable_variants() if name == "call_variants" else proc.enable(STAGE_OF[name])
    with pytest.raises(InvalidInputError) as e:
        proc.enable(stage.key)
    assert str(e.value) == stage.refusal and stage.key not in proc.stage_opt
    assert proc.stage_result(stage.key, None) is None
    proc.enable_variants() if needs == "call_variants" else proc.enable(STAGE_OF[needs])
    proc.enable(stage.key)
    assert proc.stage_opt[stage.key] == {n: d for n, d, _ in stage.options}
    # the delegates by name say the same
    fresh = CellProcessor(None, tmp_path)
    names = dict(cluster=("cluster_opt", "cluster_result"), neighbors=("neighbors_opt", "neighbor_result"),
                 clonotypes=("clonotypes_opt", "clonotype_result"))
    for key, (opt, result) in names.items():
        assert getattr(proc, opt) == proc.stage_opt.get(key) and getattr(fresh, result)(None) is None


def test_range_checkers_at_their_edges():
    from mgatk2_amd.analysis.clonotypes import check_resolution
    from mgatk2_amd.analysis.clustering import check_clones
    from mgatk2_amd.analysis.neighbors import GRAPH_MAX_K, check_neighbors, check_prune

    assert GRAPH_MAX_K + 1 == 65
    for bad in (1, 66, 0, -3):
        with pytest.raises(InvalidInputError, match=f"^neighbors must be in 2..65, got {bad}$"):
            check_neighbors(bad)
    assert check_neighbors(2) == 2 and check_neighbors(65) == 65 and type(check_neighbors(np.int64(7))) is int
    for bad in (np.nextafter(1.0, 2.0), float("nan"), -np.nextafter(0.0, 1.0), -1.0, float("inf")):
        with pytest.raises(InvalidInputError, match=r"^prune must be in \[0, 1\], got "):
            check_prune(bad)
    for ok in (-0.0, 0, 1, 1.0, 1 / 15):
        assert check_prune(ok) == ok and type(check_prune(ok)) is float
    for bad in (0, 0.0, -1, float("inf"), -float("inf"), float("nan")):
        with pytest.raises(InvalidInputError, match="^the resolution must be finite and above 0, got "):
            check_resolution(bad)
    tiny = np.nextafter(0.0, 1.0)  # the smallest positive double
    assert check_resolution(tiny) == tiny > 0 and check_resolution(1) == 1.0
    assert check_resolution(sys.float_info.max) == sys.float_info.max and math.isfinite(check_resolution(2))
    for bad in (0, -1):
        with pytest.raises(InvalidInputError, match=f"^clones must be at least 1, got {bad}$"):
            check_clones(bad)
    assert check_clones(None) is None and check_clones(1) == 1 and type(check_clones(np.int64(4))) is int


def test_every_layer_says_the_checker_s_words(tmp_path):
    """A value out of range is refused in the checker's own words by the analysis, the processor,
    the pipeline and (for the one range click's types leave to it) the command line."""
    from mgatk2_amd import cli as cli_mod
    from mgatk2_amd.analysis import cluster_heteroplasmy, find_clonotypes, min_shared_for, neighbor_graph
    from mgatk2_amd.pipeline import MtDNAPipeline
    from mgatk2_amd.processing.processors import CellProcessor

    af = np.zeros((3, 4))
    on = dict(call_variants=True, neighbors=10)
    proc = CellProcessor(None, tmp_path)
    proc.enable_variants()
    proc.enable("neighbors")
    pipe = lambda **kw: MtDNAPipeline("no.bam", ["A"], tmp_path, **kw)  # noqa: E731
    nan = float("nan")
    cases = [
        ("neighbors must be in 2..65, got 66",
         [lambda: neighbor_graph(af, neighbors=66), lambda: proc.enable("neighbors", neighbors=66),
          lambda: pipe(**dict(on, neighbors=66))]),
        ("prune must be in [0, 1], got 1.5",
         [lambda: neighbor_graph(af, prune=1.5), lambda: min_shared_for(3, 1.5),
          lambda: proc.enable("neighbors", prune=1.5), lambda: pipe(**on, snn_prune=1.5)]),
        ("the resolution must be finite and above 0, got nan",
         [lambda: find_clonotypes(None, resolution=nan), lambda: proc.enable("clonotypes", resolution=nan),
          lambda: pipe(**on, clonotypes=True, clonotype_resolution=nan)]),
        ("clones must be at least 1, got 0",
         [lambda: cluster_heteroplasmy(af, clones=0), lambda: proc.enable("cluster", clones=0),
          lambda: pipe(call_variants=True, cluster=True, clones=0)]),
    ]
    for text, calls in cases:
        for call in calls:
            with pytest.raises(InvalidInputError) as e:
                call()
            assert str(e.value) == text
    v = (True, 5, 0.65, 0.01, False, 10, 1)  # the variant options, as _variant_args takes them
    with pytest.raises(cli_mod.click.UsageError) as e:
        cli_mod._variant_args(*v, neighbors=5, clonotypes=True, clonotype_resolution=float("inf"))
    assert e.value.message == "--clonotype-resolution: the resolution must be finite and above 0, got inf"
    got = cli_mod._variant_args(*v, cluster=True, clones=2, neighbors=7, clonotypes=True, clonotype_resolution=2)
    assert {k: got[k] for k in VALUES if k in got} == dict(call_variants=True, cluster=True, clones=2, neighbors=7,
                                                          clonotypes=True, clonotype_resolution=2.0)


def test_the_command_line_declares_the_checker_s_bound():
    from mgatk2_amd import cli as cli_mod
    from mgatk2_amd.analysis.neighbors import GRAPH_MAX_K

    for cmd in (cli_mod.run, cli_mod.tenx, cli_mod.call):
        kind = next(p for p in cmd.params if p.name == "neighbors").type
        assert (kind.min, kind.max) == (2, GRAPH_MAX_K + 1)


def test_the_command_line_starts_without_numpy_or_the_analyses():
    code = ("import sys, mgatk2_amd.cli\n"
            "heavy = [m for m in sys.modules if m == 'numpy' or m.startswith(('mgatk2_amd.analysis', "
            "'mgatk2_amd.engine', 'mgatk2_amd.pipeline', 'mgatk2_amd.processing'))]\n"
            "assert not heavy, heavy\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
