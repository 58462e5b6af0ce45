"""HybridIndex.search_dev_begin / search_dev_end with one graph walk and one IVF chain per group of batches in flight
(DESIGN.md section 9o.1).  The scenarios live in _groups_child.py; the expected value of every comparison is the blocking
search_dev of the same batch on the same index (ids, hit counts, distance bits), and the number of traversal launches
says whether one walk really served the group.  Here they run at the default group sizes; the last test runs all of
them again in fresh processes under the switches, which the library reads once."""
import os
import subprocess
import sys

import pytest

import fvdb_import
import _groups_child as gc

pytestmark = pytest.mark.gpu

DEFAULT = (2, 2)  # walks, chains: HybridIndex::group_sizes() without a switch


@pytest.fixture(scope="module")
def env():
    e = gc.make_env(fvdb_import.load(), *DEFAULT)
    yield e
    del e.g
    e.ctx.close()


@pytest.mark.parametrize("scenario", gc.SCENARIOS, ids=lambda s: s.__name__[2:])
def test_default_sizes(env, scenario):
    scenario(env)


# Where the graph's slots do not run a joint walk as a device kernel, walks are not grouped (the chains still are): a
# dimension that is no multiple of 4, and the host walk.  The joint block is then never searched from another stream.
# (The restart-counter scenario is about joint walks and is left to the grouped runs: at d = 30 a batch begun in slot 0 is
# walked a second time when a later slot's end borrows slot 0 first, in this commit's parent as well, and is counted twice.)
UNGROUPED = [gc.s_reference, gc.s_groups_of_unequal_batches, gc.s_incomplete_groups, gc.s_launching_slot_reused,
             gc.s_begin_that_cannot_join, gc.s_pipelined]


@pytest.fixture(scope="module", params=[dict(d=30), dict(device=False)], ids=["d=30", "host-walk"])
def env_ungrouped(request):
    e = gc.make_env(fvdb_import.load(), *DEFAULT, **request.param)
    yield e
    del e.g
    e.ctx.close()


@pytest.mark.parametrize("scenario", UNGROUPED, ids=lambda s: s.__name__[2:])
def test_walks_that_do_not_group(env_ungrouped, scenario):
    scenario(env_ungrouped)


@pytest.mark.parametrize("setting,sizes", [({"FVDB_HYBRID_GROUP": "1"}, (1, 2)), ({"FVDB_HYBRID_GROUP": "2"}, (2, 2)),
                                           ({"FVDB_HYBRID_GROUP": "4,2"}, (4, 2)), ({"FVDB_HYBRID_GROUP": "2,4"}, (2, 4)),
                                           ({"FVDB_HYBRID_PAIR": "0"}, (1, 1))],
                         ids=["group=1", "group=2", "group=4,2", "group=2,4", "pair=0"])
def test_under_the_switches(setting, sizes):
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_groups_child.py")
    env_ = {k: v for k, v in os.environ.items() if k not in ("FVDB_HYBRID_GROUP", "FVDB_HYBRID_PAIR")}
    r = subprocess.run([sys.executable, child, str(sizes[0]), str(sizes[1])], env=dict(env_, **setting), timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("ok s_") == len(gc.SCENARIOS)
