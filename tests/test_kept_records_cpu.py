"""The kept per-cluster read-back tables on the CPU (no GPU): perception_amd/csrc/kept_records.hpp through its stand-alone program
kept_records_check.  KeptRecords is what cd_get_cluster_plane_stats / _coarse_stats / _reject_stats / _shape_frames answer from;
every case below is a script of its operations, and the program prints what each read returns."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "perception_amd", "csrc")
EXE = os.path.join(CSRC, "kept_records_check")
INVALID_ARG = -1      # cuboid_hip.h
INVALID = [INVALID_ARG, []]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.run(["make", "-C", CSRC, "kept_records_check"], check=True, stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("kept_records")
    count = [0]

    def go(*lines):
        """the script through the program -> one [return, ids written] per read; every record written was whole and the rest of
        the buffer untouched; the last element of a read is valid() at that point"""
        count[0] += 1
        path = os.path.join(str(d), "script%d.txt" % count[0])
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([EXE, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (lines, r.stderr)
        reads = json.loads(r.stdout)
        assert all(whole == 1 for _, _, whole, _ in reads), reads
        assert all(valid == 1 for got, _, _, valid in reads if got != INVALID_ARG), reads
        go.valid = [valid for _, _, _, valid in reads]
        return [[got, ids] for got, ids, _, _ in reads]
    return go


def test_nothing_to_read_before_a_publish(run):
    assert run("read 0 0 4", "begin 3", "read 0 0 4", "assign 1 2", "read 0 0 4") == [INVALID] * 3
    assert run.valid == [0, 0, 0]


INDEX = ("begin 5", "keep 0 10", "keep 1 11", "keep 2 12", "keep 3 13", "keep 4 14", "publish 0 2 2 5")


def test_windows_of_a_frame(run):
    got = run(*INDEX, "read 0 0 8", "read 1 0 8", "read 2 0 8", "read 2 1 5", "read 2 3 5", "read 3 0 8",
              "read 2 0 2", "read 2 2 1", "read 0 1 1", "read 2 2147483647 5")
    assert got == [[2, [10, 11]], [0, []], [3, [12, 13, 14]], [2, [13, 14]], [0, []], INVALID,
                   [2, [12, 13]], [1, [14]], [1, [11]], [0, []]]


def test_arguments(run):
    got = run(*INDEX, "read 0 0 0 null", "read 0 0 1 null", "read 0 0 0", "read -1 0 1", "read 0 -1 1", "read 0 0 -1", "read -1 0 0 null",
              "read 2147483647 0 1")
    assert got == [[0, []], INVALID, [0, []], INVALID, INVALID, INVALID, INVALID, INVALID]


def test_no_cluster_at_all(run):
    assert run("begin 0", "publish 0 0", "read 0 0 4", "read 1 0 4") == [[0, []], INVALID]
    assert run.valid == [1, 1]
    assert run("begin 0", "publish 0 0 0 0", "read 0 0 4", "read 2 0 4", "read 3 0 4") == [[0, []], [0, []], INVALID]


def test_keep_changes_one_slot(run):
    got = run("begin 4", "publish 0 4", "read 0 0 4", "keep 2 7", "read 0 0 4", "keep 0 9", "keep 2 8", "read 0 0 4")
    assert got == [[4, [0, 0, 0, 0]], [4, [0, 0, 7, 0]], [4, [9, 0, 8, 0]]]


def test_begin_sizes_to_the_clusters(run):
    # max(ncl, 1) default records: an index that reaches past them is refused
    assert run("begin 3", "publish 0 3", "read 0 0 8", "publish 0 4", "read 0 0 8") == [[3, [0, 0, 0]], INVALID]
    assert run("begin 0", "publish 0 1", "read 0 0 8", "publish 0 2", "read 0 0 8") == [[1, [0]], INVALID]


def test_assign_all(run):
    assert run("assign 5 6 7", "publish 0 1 3", "read 0 0 8", "read 1 0 8") == [[1, [5]], [2, [6, 7]]]
    # n = 0 after a larger table: empty, a published empty frame answers 0, an index into the old records is refused
    got = run("assign 5 6 7", "publish 0 3", "read 0 0 8", "assign", "publish 0 0", "read 0 0 8", "publish 0 1", "read 0 0 8")
    assert got == [[3, [5, 6, 7]], [0, []], INVALID]
    assert run("assign", "publish 0 0", "read 0 0 8", "read 1 0 8") == [[0, []], INVALID]


def test_publish_single(run):
    assert run(*INDEX, "single 42", "read 0 0 8", "read 0 1 8", "read 1 0 8", "read 0 0 0 null") == [[1, [42]], [0, []], INVALID, [0, []]]


def test_invalidate(run):
    got = run(*INDEX, "read 0 0 1", "invalidate", "read 0 0 1", "read 1 0 1", "single 3", "read 0 0 1", "invalidate", "read 0 0 1",
              "begin 2", "read 0 0 1", "keep 1 4", "publish 0 0 2", "read 1 0 8", "read 0 0 8")
    assert got == [[1, [10]], INVALID, INVALID, [1, [3]], INVALID, INVALID, [2, [0, 4]], [0, []]]
    assert run.valid == [1, 0, 0, 1, 0, 0, 1, 1]


def test_an_index_that_does_not_describe_the_records(run):
    # past the records, descending, negative: INVALID_ARG, never a read outside the table (the sanitizer build would say)
    assert run("begin 3", "publish 0 2 4", "read 0 0 8", "read 1 0 8") == [[2, [0, 0]], INVALID]
    assert run("begin 3", "publish 0 3 2", "read 0 0 8", "read 1 0 8") == [[3, [0, 0, 0]], INVALID]
    assert run("begin 3", "publish -1 2 3", "read 0 0 8", "read 1 0 8") == [INVALID, [1, [0]]]
    assert run("begin 3", "publish 0 2147483647", "read 0 0 8") == [INVALID]
    assert run("begin 3", "publish", "read 0 0 8") == [INVALID]
    assert run("begin 3", "publish 0", "read 0 0 8") == [INVALID]
