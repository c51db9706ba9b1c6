"""Small filesystem helpers of the reference's utils/system.py, and where a model directory keeps its newest state."""
import os


def mkdir_p(folder_path):
    os.makedirs(folder_path, exist_ok=True)


def search_for_max_interation(folder):   # (sic: the reference's spelling)
    return max(int(name.split("_")[-1]) for name in os.listdir(folder))


def model_ply(path):
    """The PLY itself, or <dir>/point_cloud/iteration_<newest>/point_cloud.ply of a model directory."""
    if os.path.isfile(path):
        return path
    pc = os.path.join(path, "point_cloud")
    its = [int(d.split("_")[-1]) for d in os.listdir(pc) if d.startswith("iteration_")] if os.path.isdir(pc) else []
    if not its:
        raise FileNotFoundError(f"{path}: neither a PLY file nor a model directory with point_cloud/iteration_N")
    return os.path.join(pc, f"iteration_{max(its)}", "point_cloud.ply")
