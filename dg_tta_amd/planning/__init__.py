"""`dgtta plan`: the dataset fingerprint (fingerprint.py, GPU) and the experiment planner (planner.py, host) - the first command
of the nnU-Net workflow, so that `dgtta pretrain` can start from a raw labelled dataset alone."""
