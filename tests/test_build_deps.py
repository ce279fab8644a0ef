"""seqlib_amd/build.py decides what to compile from the dependency files the compiler writes beside every object (-MMD -MF): the parser of those files and the
staleness rule, on hand-written files.  No compiler runs here."""
import os

from seqlib_amd import build as b

DEP = """build/slx_cov.hip.o: csrc/slx_cov.hip \\
  csrc/slx_internal.h csrc/slx_hip.h \\
  ../include/seqlib_amd_cov.h \\
 csrc/dev\\ cov.h
"""


def test_continuation_lines_and_the_target():
    assert b.parse_depfile(DEP) == ["csrc/slx_cov.hip", "csrc/slx_internal.h", "csrc/slx_hip.h", "../include/seqlib_amd_cov.h", "csrc/dev cov.h"]


def test_one_line_no_prerequisites_and_nothing():
    assert b.parse_depfile("a.o: a.c b.h\n") == ["a.c", "b.h"]
    assert b.parse_depfile("a.o:\n") == [] and b.parse_depfile("") == [] and b.parse_depfile("\n\n") == []
    # the phony rules of -MP name no prerequisites; two rules give the files of both
    assert b.parse_depfile("a.o: a.c \\\n b.h\nb.h:\nc.o: c.c\n") == ["a.c", "b.h", "c.c"]


def files(tmp_path, dep_names):
    obj, dep = tmp_path / "x.o", tmp_path / "x.o.d"
    paths = [tmp_path / n for n in dep_names]
    for i, p in enumerate(paths):
        p.write_text("")
        os.utime(p, (1000 + i, 1000 + i))
    obj.write_text("")
    os.utime(obj, (2000, 2000))
    dep.write_text("%s: %s\n" % (obj, " \\\n  ".join(str(p) for p in paths)))
    return obj, dep, paths


def test_fresh_when_every_dependency_is_older(tmp_path):
    obj, dep, _ = files(tmp_path, ["x.hip", "a.h", "b.h"])
    assert not b.stale(str(obj), str(dep))


def test_stale_without_the_object_or_without_its_dependency_file(tmp_path):
    obj, dep, _ = files(tmp_path, ["x.hip", "a.h"])
    dep.unlink()
    assert b.stale(str(obj), str(dep))
    obj2, dep2, _ = files(tmp_path, ["y.hip"])
    obj2.unlink()
    assert b.stale(str(obj2), str(dep2))


def test_stale_when_one_dependency_is_newer_and_only_then(tmp_path):
    obj, dep, paths = files(tmp_path, ["x.hip", "a.h", "b.h"])
    os.utime(paths[2], (2001, 2001))          # the last name of a continued rule
    assert b.stale(str(obj), str(dep))
    os.utime(paths[2], (2000, 2000))          # as old as the object: not newer
    assert not b.stale(str(obj), str(dep))
    (tmp_path / "unrelated.h").write_text("")          # a file the object was not made from
    assert not b.stale(str(obj), str(dep))


def test_stale_when_a_dependency_is_gone(tmp_path):
    obj, dep, paths = files(tmp_path, ["x.hip", "a.h"])
    paths[1].unlink()
    assert b.stale(str(obj), str(dep))
