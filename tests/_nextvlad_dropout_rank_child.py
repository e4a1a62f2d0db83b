"""One rank of tests/test_gpu_nextvlad_dropout.py::test_train_main_two_ranks_drop_different_elements: train.main on the
arguments after the output path (the launcher's environment is set by the test), then this rank's key and the mask of its last
forward - (Y_bf != 0) of the tower train.main built - saved as an .npz."""
import sys

import numpy as np
import torch

from efficientvideoclassification_youtube8m_amd import train

if __name__ == "__main__":
    res = train.main(sys.argv[2:])
    tw = res["graph"].tower
    mask = (tw.Y_bf[:tw.B].view(torch.int16) != 0).cpu().numpy()
    np.savez(sys.argv[1], mask=mask, rank=tw.rank, seed=tw.dropout_seed, global_step=res["graph"].global_step, K=tw.Kc, D=tw.D)
