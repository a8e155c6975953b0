"""`cd index && python decode_indices.py --ckpt_path ... --index_file ...` -- the tuples of an index file back to embeddings, and
what they cost in reconstruction loss (the reference has no such command), forwarded to lc-rec_amd/decode_indices.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lcrec_amd.decode_indices import main  # noqa: E402

if __name__ == "__main__":
    main()
