"""`cd index && python query_indices.py --ckpt_path ... --index_file ... --queries Q.npy` -- which catalogue items an embedding
lands on (the reference has no such command), forwarded to lc-rec_amd/query_indices.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lcrec_amd.query_indices import main  # noqa: E402

if __name__ == "__main__":
    main()
