"""Golden parse tests against the reference's own Polyaxonfiles: every ``*_content`` spec of
polyaxon/factories/fixtures.py:11-461 and every complete example in docs/templates/polyaxonfile_specification.

The Polyaxonfiles themselves (YAML settings, nothing executable) are stored in tests/golden/
reference_polyaxonfiles.json: ``fixtures`` maps every ``*_content`` name to its YAML, ``doc_examples`` lists the
complete ``version:`` + ``kind:`` YAML blocks of the specification docs with the page each came from."""
import json
import os

from polyaxon_amd.spec import specification_for
from polyaxon_amd.spec.specification import GroupSpecification, Kinds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_polyaxonfiles.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _fixture_strings():
    return dict(_golden()["fixtures"])


def test_every_reference_fixture_parses():
    specs = _fixture_strings()
    assert len(specs) >= 13
    kinds = {}
    for name, content in specs.items():
        spec = specification_for(content)
        kinds[name] = spec.kind
    assert kinds["experiment_group_spec_content"] == Kinds.GROUP
    assert kinds["build_spec_content"] == Kinds.BUILD
    assert kinds["notebook_spec_content"] == Kinds.NOTEBOOK and kinds["tensorboard_spec_content"] == Kinds.TENSORBOARD
    assert kinds["job_spec_content"] == Kinds.JOB


def test_fixture_semantics():
    s = _fixture_strings()
    g = specification_for(s["experiment_group_spec_content"])
    assert isinstance(g, GroupSpecification) and g.search_algorithm == "grid_search" and g.tags == ["fixtures"]
    assert g.matrix_space == 5  # logspace 0.01:0.1:5

    hb = specification_for(s["experiment_group_spec_content_hyperband"]).hptuning.hyperband
    assert hb is not None and hb.max_iter > 0 and hb.eta > 1 and hb.resource.name and hb.metric.name

    es = specification_for(s["experiment_group_spec_content_early_stopping"]).hptuning.early_stopping
    assert es and all(r.metric and r.optimization in ("maximize", "minimize") for r in es)

    bo = specification_for(s["experiment_group_spec_content_bo"]).hptuning.bo
    assert bo is not None and bo.n_iterations > 0 and bo.utility_function.acquisition_function in ("ucb", "ei", "poi")

    res = specification_for(s["exec_experiment_resources_content"])
    cluster, distributed = res.cluster_def
    assert distributed and sum(cluster.values()) > 1
    assert res.total_resources is not None

    refs = specification_for(s["exec_experiment_outputs_refs_content"])
    assert refs.environment.outputs.get("jobs") or refs.environment.outputs.get("experiments")

    job = specification_for(s["job_spec_resources_content"])
    assert job.resources is not None
    build = specification_for(s["build_spec_content"])
    assert build.build.image


def _doc_yaml_blocks():
    for ex in _golden()["doc_examples"]:
        yield ex["source"], ex["yaml"]


def test_complete_doc_examples_parse():
    blocks = list(_doc_yaml_blocks())
    assert len(blocks) >= 10
    for fn, block in blocks:
        spec = specification_for(block)
        assert spec.kind in Kinds.VALUES, fn
