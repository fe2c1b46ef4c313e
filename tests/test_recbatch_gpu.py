"""The recording-batch object on the GPU (recbatch.py, ops.py, diarize.py): the per-recording forms of
ops.score_dense and ops.score_dense_q against the global forms, bit for bit, and the uploads of the batch table one diarize() call
makes.  Three recordings of 1, 17 and 40 windows, D = L = 8: one row, one past the 16-row tile, several tiles."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pca_ref as P  # noqa: E402

NS, L = (1, 17, 40), 8
RO = np.concatenate([[0], np.cumsum(NS)]).astype(np.int64)


@pytest.fixture(scope="module")
def env():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize, ops
    from pytorch_kaldi_resnet_amd.recbatch import RecBatch
    return {"diarize": diarize, "ops": ops, "RecBatch": RecBatch}


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_per_recording_forms_equal_the_global_forms(env):
    ops, R = env["ops"], len(NS)
    rng = np.random.RandomState(4)
    U, g, k, K = up(rng.randn(RO[-1], L)), rng.uniform(0.1, 1.0, L), rng.uniform(0.1, 1.0, L), 0.37
    rec = env["RecBatch"](RO)
    q = ops.score_dense_q(U, up(k), -0.5)
    for r in (rec, RO):                                             # the batch object and the raw offsets
        q_rec = ops.score_dense_q(U, up(np.tile(k, (R, 1))), -0.5, r)
        assert q.cpu().numpy().tobytes() == q_rec.cpu().numpy().tobytes()
        one, mo = ops.score_dense(U, r, q, up(g), K)
        per, mo2 = ops.score_dense(U, r, q, up(np.tile(g, (R, 1))), up(np.full(R, K)))
        assert mo.tolist() == mo2.tolist() == [0, 1, 290, 1890] and one.numel() == 1890
        assert one.cpu().numpy().tobytes() == per.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def case():
    """planted recordings whose projection (mean 0, identity transform) the scoring sees, each within section 6p's conditions at
    E = 0.5, so both back ends must retain the same dimensions"""
    model = P.planted(8, L, 1, seed=50)[2]
    zs = [P.planted(n, L, min(2, n), seed=30 + i)[0] for i, n in enumerate(NS)]
    for z in zs[1:]:
        P.assert_conditions(P.pca_ref(z, model, 0.5, np.longdouble), 0.5, len(z))
    emb, segments = {}, []
    for r, z in enumerate(zs):
        for i, row in enumerate(z):
            key = "rec%d-%04d" % (r, i)
            emb[key] = row.astype(np.float64)
            segments.append((key, "rec%d" % r, 0.25 * i, 0.25 * i + 0.5))
    kw = dict(kind="plda", reco2num_spk={"rec%d" % r: 2 for r in range(len(NS))}, target_energy=0.5, vbx={}, mean=np.zeros(L),
              transform=np.eye(L), plda=model)
    return emb, segments, kw


def _count_uploads(env, monkeypatch):
    RecBatch, sizes = env["RecBatch"], []
    upload = RecBatch._upload

    def counted(self, device):
        sizes.append(self.R)
        return upload(self, device)

    monkeypatch.setattr(RecBatch, "_upload", counted)
    return sizes


def test_one_diarize_call_uploads_its_table_once(env, case, monkeypatch):
    diarize = env["diarize"]
    emb, segments, kw = case
    host = diarize.diarize(emb, segments, backend="host", **kw)
    sizes = _count_uploads(env, monkeypatch)
    dev = diarize.diarize(emb, segments, backend="hip", **kw)
    assert sizes == [3]                                             # the PCA, the rows, q, the scores, the clustering and VBx: one table
    assert dev["labels"].tolist() == host["labels"].tolist() and dev["pca_dim"] == host["pca_dim"] and dev["rttm"] == host["rttm"]
    assert dev["ahc_labels"].tolist() == host["ahc_labels"].tolist() and len(dev["pca_dim"]) == 3 and dev["pca_dim"][0] == L
    assert host["rec_off"].tolist() == RO.tolist() and dev["mat_off"].tolist() == [0, 1, 290, 1890]
    # a budget that splits: 4672 bytes per recording of the PCA (one per launch: 3 sub-batches), 8 n^2 of the clustering (8 + 2312 |
    # 12800: 2), and with two states at most 56 per row + 128 per recording of VBx (184 + 1080 | 2368: 2); the whole batch's table
    # serves the three row kernels and the scores
    assert 8 * (env["ops"].pca_plda_ws_elems(np.array([0, 1]), L) - 1) == 4672 and dev["vbx_pi"].shape[1] == 2
    del sizes[:]
    split = diarize.diarize(emb, segments, backend="hip", ws_budget_bytes=3000, **kw)
    assert sorted(sizes) == [1, 1, 1, 1, 1, 2, 2, 3]
    assert split["labels"].tolist() == host["labels"].tolist() and split["pca_dim"] == host["pca_dim"] and split["rttm"] == host["rttm"]
    assert split["vbx_elbo"].tobytes() == dev["vbx_elbo"].tobytes() and split["merge_cost"].tobytes() == dev["merge_cost"].tobytes()
