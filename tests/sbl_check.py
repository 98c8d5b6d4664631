"""Checker run by tests/test_sbl_reference.py::test_gpu_with_device_buffers (TEST INFRASTRUCTURE): the checks of that file that hand device buffers of
the caller to libssgpu on the MI355X -- ssg_markdup_sig_dev, ssg_hotpath_dev_ex -- with the buffers in torch tensors, in a process of their own because torch
must initialise its HIP runtime before libssgpu is loaded (as in bench.py and tests/hotpath_check.py).  argv[1] = owner | simulated150 | simulated250."""
import os
import sys

import torch

torch.cuda.init()
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tools"))
import test_sbl_reference as T  # noqa: E402
from speedseq_amd import capi  # noqa: E402

lib = capi.Lib()


def to_dev(a):
    t = torch.from_numpy(a).cuda()
    return t, t.data_ptr()


what = sys.argv[1]
if what == "owner":
    T.owner_side_everything(lib, to_dev)
    r = ()
else:
    r = (T.hold_simulated(lib, 3000, 1000, int(what[len("simulated"):]), to_dev),)
torch.cuda.synchronize()
print("sbl ok", *r)
