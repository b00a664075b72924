"""The load loops of the row-streaming kernels, every one of them (dsp_reduce.hip, dsp_thresh.hip, dsp_hist.hip, dsp_extrema.hip):
rows of every length at which a group of loads begins or ends, flat but for one sample on a boundary of the loop, on the 16-byte path and on
the sample-per-lane path, in every row type the kernel takes.  Bit for bit against NumPy and the case books' models
(tests/row_stream_cases.py; test_row_stream_cases_cpu.py vouches for the list)."""
import numpy as np
import pytest

import row_stream_cases as rs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kernel,tag,path", rs.families())
def test_a_sample_on_every_boundary_of_the_loop(kernel, tag, path):
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray

    n_launches = 0
    for c in rs.cases(kernel, tag, path):
        prog, kernel_name = c.program()
        ch = Chain(prog, c.name, c.loop)
        assert ch.kernel_name == kernel_name, (c.name, ch.kernel_name)
        want = c.expected()
        bufs = {"wf": DeviceArray.from_numpy(c.block())}
        for name, a in c.inputs().items():
            bufs[name] = DeviceArray.from_numpy(a)
        for name, a in want.items():
            bufs[name] = DeviceArray.from_numpy(np.full(a.shape, 7, dtype=a.dtype))
        ch.execute(bufs, len(c.rows))
        ch.check()
        for name, a in want.items():
            got = bufs[name].to_numpy()
            assert got.dtype == a.dtype and got.shape == a.shape, (c.name, name)
            assert np.array_equal(got, a, equal_nan=True), (c.name, name, got, a)
        ch.close()
        n_launches += 1
    assert n_launches == len(rs.all_lengths(kernel, tag, path)) - len(rs.left_out(kernel, tag, path)) > 0
