"""The two host helpers every raw call goes through before a pointer reaches a kernel (robosimgs_amd/_lib.py):
check_tensor and aligned_workspace.  CPU tensors only: neither touches a device or the library.
"""
import pytest
import torch

from robosimgs_amd._lib import aligned_workspace, check_tensor

CPU = torch.device("cpu")


def test_check_tensor_accepts_what_a_kernel_can_read():
    t = torch.zeros(5, 3)
    for shape in ((5, 3), (-1, 3), (5, -1), (-1, -1)):
        check_tensor("means", t, torch.float32, shape)
    check_tensor("means", t, torch.float32, (5, 3), CPU)
    check_tensor("ids", torch.zeros(0, dtype=torch.int32), torch.int32, (-1,))
    check_tensor("ids", torch.zeros(8, dtype=torch.int32)[2:], torch.int32, (6,))         # an offset view is contiguous


@pytest.mark.parametrize("name,bad,dtype,shape", (
    ("not_a_tensor", [[0.0] * 3] * 5, torch.float32, (5, 3)),
    ("nothing", None, torch.float32, (5, 3)),
    ("rank", torch.zeros(15), torch.float32, (5, 3)),
    ("rank_any", torch.zeros(5, 3, 1), torch.float32, (-1, 3)),
    ("extent", torch.zeros(4, 3), torch.float32, (5, 3)),
    ("extent_any", torch.zeros(5, 2), torch.float32, (-1, 3)),
    ("dtype", torch.zeros(5, 3, dtype=torch.float64), torch.float32, (5, 3)),
    ("int_dtype", torch.zeros(7, dtype=torch.int64), torch.int32, (-1,)),
    ("strided", torch.zeros(10, 3)[::2], torch.float32, (5, 3)),
    ("transposed", torch.zeros(3, 5).t(), torch.float32, (5, 3)),
))
def test_check_tensor_refuses_and_names_the_argument(name, bad, dtype, shape):
    with pytest.raises(ValueError) as e:
        check_tensor(name, bad, dtype, shape)
    msg = str(e.value)
    assert msg.startswith(name + " must be a contiguous " + str(dtype)[6:] + " tensor"), msg
    assert "got " in msg and (type(bad).__name__ in msg if not torch.is_tensor(bad) else str(list(bad.shape)) in msg), msg


def test_check_tensor_refuses_another_device():
    with pytest.raises(ValueError) as e:
        check_tensor("frame", torch.zeros(2, 2), torch.float32, (2, 2), torch.device("meta"))
    assert str(e.value).startswith("frame must be") and "on meta" in str(e.value) and "on cpu" in str(e.value)


def test_aligned_workspace_finds_the_first_aligned_byte():
    buf = torch.zeros(4096, dtype=torch.uint8)
    for start in (1, 3, 255, 256, 257):
        ws = buf[start:]
        assert ws.data_ptr() == buf.data_ptr() + start
        got, pad = aligned_workspace(ws, 1000, CPU)
        assert got is ws and 0 <= pad < 256 and (ws.data_ptr() + pad) % 256 == 0
    exact = buf[1:1 + (-(buf.data_ptr() + 1) % 256) + 1000]              # exactly pad + need bytes: the size is not its to judge
    assert aligned_workspace(exact, 1000, CPU)[0] is exact
    rows = torch.zeros(4, 512, dtype=torch.uint8)                       # rank and device are the call site's to judge too
    assert aligned_workspace(rows, 1000, torch.device("meta"))[0] is rows


def test_aligned_workspace_allocates_need_plus_256():
    for need in (0, 1, 1000):
        ws, pad = aligned_workspace(None, need, CPU)
        assert ws.dtype == torch.uint8 and ws.device == CPU and tuple(ws.shape) == (need + 256,)
        assert (ws.data_ptr() + pad) % 256 == 0 and ws.numel() - pad >= need


@pytest.mark.parametrize("bad", (torch.zeros(1024, dtype=torch.int8), torch.zeros(2048, dtype=torch.uint8)[::2],
                                 torch.zeros(256, dtype=torch.float32), bytearray(1024)))
def test_aligned_workspace_refuses_what_is_not_contiguous_uint8(bad):
    with pytest.raises(ValueError) as e:
        aligned_workspace(bad, 16, CPU)
    assert str(e.value).startswith("workspace must be a contiguous uint8 tensor")
