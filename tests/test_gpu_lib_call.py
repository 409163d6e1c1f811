"""_lib.call on the device: what the entry is handed (a recording callable stands in for it), which stream it is handed under
``torch.cuda.stream``, how its return code is raised, and one real entry through it on either side of a block boundary."""
import pytest
import torch

from sequoia_pub_amd import _lib

pytestmark = pytest.mark.gpu


class _Recorder:
    def __init__(self, rc=0):
        self.rc, self.args, self.device = rc, None, None

    def __call__(self, *args):
        self.args, self.device = args, torch.cuda.current_device()
        return self.rc


def test_the_entry_sees_addresses_the_workspace_pair_and_the_current_stream():
    x = torch.zeros(16, device="cuda:0")
    rec = _Recorder()
    _lib.call(rec, x.device, x, 3, None, workspace=64)
    assert rec.args[:3] == (x.data_ptr(), 3, None) and len(rec.args) == 6
    assert isinstance(rec.args[3], int) and rec.args[3] != 0 and rec.args[4] == 64
    assert (rec.args[5].value or 0) == torch.cuda.current_stream().cuda_stream     # (a null handle reads back as None)
    assert rec.device == x.device.index
    side = torch.cuda.Stream(device=x.device)
    with torch.cuda.stream(side):
        _lib.call(rec, x.device, x, 3, None, workspace=64)
    assert rec.args[:3] == (x.data_ptr(), 3, None) and rec.args[4] == 64
    assert rec.args[5].value == side.cuda_stream and side.cuda_stream != 0
    ws, extra = torch.empty(32, dtype=torch.uint8, device=x.device), (object(), 2)
    _lib.call(rec, x.device, x[4:], workspace=ws, after=extra)               # a kept workspace; arguments behind the stream as they are
    assert rec.args[:3] == (x.data_ptr() + 16, ws.data_ptr(), 32) and rec.args[4:] == extra


def test_return_codes_are_raised():
    x = torch.zeros(1, device="cuda:0")
    with pytest.raises(_lib.SequoiaHipArgError):
        _lib.call(_Recorder(_lib.SQ_ERR_ARG), x.device, x)
    assert _lib.SQ_ERR_ARG == -1
    with pytest.raises(_lib.SequoiaHipError) as e:
        _lib.call(_Recorder(-3), x.device, x)
    assert not isinstance(e.value, ValueError)


@pytest.mark.parametrize("n", [8, 1025])
def test_a_real_entry_on_the_current_and_on_a_side_stream(n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to("cuda:0")
    want = x.to(torch.bfloat16)
    got = torch.empty(n, dtype=torch.bfloat16, device=x.device)
    _lib.call("sq_cast_f32_to_bf16", x.device, x, got, n)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    side, got2 = torch.cuda.Stream(device=x.device), torch.zeros(n, dtype=torch.bfloat16, device=x.device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.call(_lib.lib().sq_cast_f32_to_bf16, x.device, x, got2, n)
    side.synchronize()
    assert torch.equal(got2.view(torch.int16), want.view(torch.int16))
