"""The inputs of tests/test_gpu_commit_fq.py really produce the admission cases they are meant to (CPU oracle only)."""
import numpy as np

from helpers import profile
from koordinator_amd import abi
from test_gpu_commit_fq import assert_edges, edge_workload, np_followup


def test_edge_workload_produces_every_admission_case(oracle_lib):
    nodes, pods, q = edge_workload()
    for batch in (64, 7):
        cfg = profile(quota=True, check_parent=True, batch_pods=batch).to_ks_config()
        orc = oracle_lib.Oracle(cfg, nodes.copy(), q.copy(), nthreads=1)
        want = orc.schedule(pods)
        assert_edges(want, pods)
        s1 = np.asarray(orc.schedule(np_followup(pods))["status"])
        orc.close()
        assert (s1 == abi.KS_S_QUOTA_NONPREEMPTIBLE).any() and (s1 == abi.KS_S_SCHEDULED).any()
