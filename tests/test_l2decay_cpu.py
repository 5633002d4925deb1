"""The host side of the one-launch L2 weight decay (networks/_plumbing.py) without a GPU: which parameter lists it
takes, and the chunk table's rows."""
import torch

from wssdl_bus_amd.fast_rcnn import train_bus as T
from wssdl_bus_amd.fast_rcnn.config import cfg
from wssdl_bus_amd.networks import _plumbing as P


def test_storage_dense():
    x = torch.zeros(6, 4, 5, 3)
    assert P._storage_dense(x) and P._storage_dense(x.permute(0, 3, 1, 2)) and P._storage_dense(x.permute(3, 2, 1, 0))
    assert P._storage_dense(torch.zeros(64, 3, 7, 7).contiguous(memory_format=torch.channels_last))
    assert P._storage_dense(torch.zeros(1, 5, 1)[:, :, 0].expand(1, 5)) and P._storage_dense(torch.zeros(8)[2:5])
    assert not P._storage_dense(x[:, ::2]) and not P._storage_dense(x[:, :, :, 0])
    assert not P._storage_dense(torch.zeros(3, 1).expand(3, 4)) and not P._storage_dense(torch.zeros(0))


def test_cpu_parameters_take_the_torch_chain():
    p = [torch.nn.Parameter(torch.full((3, 2), 2.0)), torch.nn.Parameter(torch.ones(4))]
    assert not P.l2decay_usable(p) and not P.l2decay_usable([])
    loss = T.l2_weight_decay(p)
    assert type(loss.grad_fn).__name__ == "MulBackward0"
    loss.backward()
    assert torch.equal(p[0].grad, 2 * p[0].detach() * torch.tensor(0.5 * cfg.TRAIN.WEIGHT_DECAY))
    assert "WSSDL_TORCH_L2_DECAY" in P.SWITCHES


def test_chunk_table_rows():
    ps = [torch.zeros(3), torch.zeros(2 * P._L2_CHUNK + 5).view(-1, 1), torch.zeros(1), torch.zeros(P._L2_CHUNK)]
    t = P._L2Table(ps)
    rows = t.table.tolist()
    assert t.offsets == [0, 4, 4 + 2 * P._L2_CHUNK + 8, 4 + 2 * P._L2_CHUNK + 12]
    assert t.total == t.offsets[-1] + P._L2_CHUNK and t.n_chunks == len(rows) == 6
    assert [r[2] for r in rows] == [3, P._L2_CHUNK, P._L2_CHUNK, 5, 1, P._L2_CHUNK]
    assert [r[1] for r in rows] == [0, 4, 4 + P._L2_CHUNK, 4 + 2 * P._L2_CHUNK, t.offsets[2], t.offsets[3]]
    assert [r[0] for r in rows] == [ps[0].data_ptr(), ps[1].data_ptr(), ps[1].data_ptr() + 4 * P._L2_CHUNK,
                                    ps[1].data_ptr() + 8 * P._L2_CHUNK, ps[2].data_ptr(), ps[3].data_ptr()]
    # every chunk stays inside its parameter's segment of the flat buffer, and the segments do not overlap
    ends = t.offsets[1:] + [t.total]
    for p, off, end in zip(ps, t.offsets, ends):
        assert off % P._L2_ALIGN == 0 and off + p.numel() <= end
