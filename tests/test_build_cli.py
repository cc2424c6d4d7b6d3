"""`cls-build-db` (the reference's `cls build-db`, ports/cli/src/cmds/build_db.rs) on the host builder: no GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from classeq2_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "classeq2_amd", "csrc", "cls-build-db")
ARRAYS = ("bucket_key", "bucket_kmer_off", "kmer_hash", "kmer_node_off", "node_ids")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli")
    nw = json.load(open(os.path.join(GOLD, "newick_colletotrichum.json")))
    gold = json.load(open(os.path.join(GOLD, "builder_colletotrichum.json")))
    tree = d / nw["tree_name"]
    tree.write_text(nw["newick"])
    msa = d / "msa.fasta"
    msa.write_text(gold["msa_fasta"])
    return dict(dir=d, tree=str(tree), msa=str(msa), msa_text=gold["msa_fasta"].encode())


def _run(*args, cwd=None):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120, cwd=cwd)


@pytest.mark.parametrize("shift", [True, False])
def test_host_build_writes_the_in_memory_database(inputs, tmp_path, shift):
    out = tmp_path / "db.whatever"
    args = [inputs["tree"], inputs["msa"], "--host", "-k", "12", "-m", "4", "-s", "-2", "-o", str(out), "-t", "8"]
    r = _run(*(args + ([] if shift else ["--no-header-shift"])))
    assert r.returncode == 0, r.stderr
    path = tmp_path / "db.cls"  # the extension is forced to .cls (build_db.rs:72)
    assert path.exists() and not out.exists()
    assert open(path, "rb").read(4) == b"\x28\xb5\x2f\xfd"  # zstd frame
    got = engine.Tree(str(path)).flat()
    t = engine.Tree.from_newick_file(inputs["tree"], min_branch_support=-2.0)
    t.build_kmers_map(inputs["msa_text"], 12, 4, reference_header_shift=shift)
    want = t.flat()
    for f in ("nodes",) + ARRAYS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert (got.k_size, got.m_size) == (12, 4)


def test_default_output_path_and_sizes(inputs, tmp_path):
    r = _run(inputs["tree"], inputs["msa"], "--host", cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    got = engine.Tree(str(tmp_path / "classeq-database.cls")).flat()
    assert (got.k_size, got.m_size) == (35, 4)


@pytest.mark.parametrize("bad", [["-k", "0"], ["-k", "abc"], ["-k"], ["--k-size", "-3"], ["-m", "x"], ["--bogus"]])
def test_bad_arguments_exit_1_with_one_line(inputs, tmp_path, bad):
    r = _run(inputs["tree"], inputs["msa"], "--host", "-o", str(tmp_path / "x"), *bad)
    assert r.returncode == 1
    assert len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert not (tmp_path / "x.cls").exists()


def test_missing_files_exit_1_with_one_line(inputs, tmp_path):
    for args in ([inputs["tree"], str(tmp_path / "nope.fasta")], [str(tmp_path / "nope.nwk"), inputs["msa"]], [inputs["tree"]]):
        r = _run(*args, "--host", "-o", str(tmp_path / "x"))
        assert r.returncode == 1, args
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr


def test_unknown_header_exit_1_with_the_builders_message(inputs, tmp_path):
    msa = tmp_path / "bad.fasta"
    msa.write_text(">nobody\nACGTACGTACGTACGT\n>nobody2\nACGTACGTACGTAAAA\n")
    r = _run(inputs["tree"], str(msa), "--host", "-k", "12", "-o", str(tmp_path / "x"))
    assert r.returncode == 1
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and "does not match any tree leaf" in lines[0]


def test_help_lists_the_flags():
    r = _run("--help")
    assert r.returncode == 0
    for flag in ("-k, --k-size", "-m, --m-size", "-s, --min-branch-support", "-o, --output-file-path", "-t, --threads",
                 "--device", "--host", "--no-header-shift", "<TREE>", "<MSA>", "classeq-database.cls"):
        assert flag in r.stdout, flag


def test_leaves_only_map_refuses_the_database_format(inputs, tmp_path):
    """A leaves-only map (host builder, CLS_BUILD_LEAVES_ONLY) is the node sets reduced to leaves; the reference's file
    holds explicit sets, so saving it with the map is refused while only_tree still works."""
    t = engine.Tree.from_newick_file(inputs["tree"], min_branch_support=-2.0)
    t.build_kmers_map(inputs["msa_text"], 12, 4)
    want = t.flat().to_leaves_only()  # (a copy: the tree's arrays are replaced below)
    lib = engine.lib()
    engine._check_host(lib.cls_tree_build_kmers_map(t._h, inputs["msa_text"], len(inputs["msa_text"]), 12, 4, 1 | 4))
    leaves = t.flat()
    assert leaves.leaves_only
    for f in ARRAYS:
        assert np.array_equal(getattr(leaves, f), getattr(want, f)), f
    with pytest.raises(engine.ClsError, match="leaves-only"):
        t.save(str(tmp_path / "db"))
    t.save(str(tmp_path / "db"), only_tree=True)
    assert (tmp_path / "db.cls").exists()
