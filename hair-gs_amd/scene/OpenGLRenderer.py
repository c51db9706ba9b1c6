"""The reference's renderer interface (scene/OpenGLRenderer.py there) over scene/mesh_renderer.py, so that code written against it
runs unchanged.  Despite the name, nothing here uses OpenGL: render() rasterizes with the contract of scene/mesh_renderer.py, on
the host (device=None) or with csrc/hgs_raster.hip (device="cuda", one upload of the meshes per setup_meshes)."""
import numpy as np

from scene.mesh_renderer import Lighting, MeshModel, render_views

__all__ = ["OpenGLModel", "OpenGLCamera", "OpenGLLighting", "OpenGLRenderer"]


class OpenGLModel(MeshModel):
    def __init__(self, vertices, colors=None, normals=None, edges=None, faces=None, model=np.eye(4), use_lighting=True,
                 line_width=1.0, ka=0.5, kd=0.5):
        super().__init__(vertices, colors=colors, normals=normals, edges=edges, faces=faces, model=model,
                         use_lighting=use_lighting, line_width=line_width, ka=ka, kd=kd)


class OpenGLCamera:
    def __init__(self, view, projection):
        self.view = np.asarray(view).astype(np.float32)
        self.projection = np.asarray(projection).astype(np.float32)


class OpenGLLighting(Lighting):
    _dark = np.array([0.0, 0.0, 0.0, 0.0])

    def __init__(self, light_pos=np.array([10, 10, 10]), diffuse_color=_dark, ambient_color=_dark, specular_color=_dark):
        super().__init__(light_pos=light_pos, diffuse_color=diffuse_color, ambient_color=ambient_color)
        self.specular_color = np.asarray(specular_color).astype(np.float32)     # (the reference's shader does not read it)


class OpenGLRenderer:
    def __init__(self, resolution, device=None):
        self.resolution = resolution          # (width, height)
        self.models = []
        self.camera = None
        self.lighting = None
        self.device = device
        self._uploads = {}

    def setup(self):
        self.setup_meshes()
        self.setup_camera()
        self.setup_lighting()

    def setup_meshes(self, idx=None):
        self._uploads = {}                    # the next device render uploads the current models again

    def setup_camera(self):
        pass

    def setup_lighting(self):
        pass

    def render(self, mesh_indices=None, background_color=(0.0, 0.0, 0.0, 1.0)):
        """uint8 [H, W, 3] RGB, image rows top-down (numpy for device=None, a device tensor otherwise)."""
        if self.camera is None:
            raise RuntimeError("OpenGLRenderer.render: no camera")
        W, H = self.resolution
        state = None
        if self.device is not None and str(self.device) != "cpu":
            from scene._raster_device import DeviceMeshes
            from scene.mesh_renderer import _Prepared
            key = None if mesh_indices is None else tuple(sorted({int(i) for i in mesh_indices}))
            if key not in self._uploads:
                self._uploads[key] = DeviceMeshes(_Prepared(self.models, mesh_indices), self.device)
            state = self._uploads[key]
        img, _ = render_views(self.models, self.camera.view, self.camera.projection, W, H, self.lighting, mesh_indices=mesh_indices,
                              background=background_color, device=self.device, _device_state=state)
        return img[0]
