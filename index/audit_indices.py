"""`cd index && python audit_indices.py --ckpt_path ... --index_file ...` -- what the tuples of an index file cost, code by code
(the reference has no such command), forwarded to lc-rec_amd/audit_indices.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lcrec_amd.audit_indices import main  # noqa: E402

if __name__ == "__main__":
    main()
