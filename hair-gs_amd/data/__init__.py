"""Dataset IO around the hot path: COLMAP sparse models, the camera infos built from them, and (data/capture.py, not
star-imported: the capture tools and the loader name it) where a capture keeps its files and how one is rewritten."""
from data.colmap import *  # noqa: F401,F403
from data.dataset_readers import *  # noqa: F401,F403
from data.eval_data import *  # noqa: F401,F403,E402
from data.head_reconstruction_data import *  # noqa: F401,F403,E402
