"""gymnasium.wrappers.RecordVideo over env.render() (render_mode="rgb_array").  gymnasium writes mp4 through
moviepy; no video encoder is available here, so the frames are written with Pillow as an animated GIF (default) or
APNG (lossless): ``video_format`` in {"gif", "apng"}."""
from __future__ import annotations

import os

VIDEO_FORMATS = {"gif": ".gif", "apng": ".png"}


def capped_cubic_video_schedule(episode_id: int) -> bool:
    """gymnasium's default episode trigger: episodes 0, 1, 8, 27, ..., 1000, then every 1000th."""
    if episode_id < 1000:
        return int(round(episode_id ** (1.0 / 3))) ** 3 == episode_id
    return episode_id % 1000 == 0


class RecordVideo:
    def __init__(self, env, video_folder: str = "videos", episode_trigger=None, step_trigger=None,
                 video_length: int = 0, name_prefix: str = "rl-video", fps: float | None = None,
                 disable_logger: bool = True, video_format: str = "gif"):
        if getattr(env, "render_mode", None) != "rgb_array":
            raise ValueError(f"RecordVideo needs render_mode='rgb_array', got {getattr(env, 'render_mode', None)!r}")
        if video_format not in VIDEO_FORMATS:
            raise ValueError(f"video_format: {video_format!r} ({' | '.join(VIDEO_FORMATS)})")
        if episode_trigger is None and step_trigger is None:
            episode_trigger = capped_cubic_video_schedule
        self.env = env
        self.video_folder = os.path.abspath(video_folder)
        os.makedirs(self.video_folder, exist_ok=True)
        self.episode_trigger, self.step_trigger = episode_trigger, step_trigger
        self.video_length = int(video_length) if video_length else 0  # 0: until the episode ends
        self.name_prefix = name_prefix
        self.disable_logger = disable_logger
        self.video_format = video_format
        if fps is None:
            dt = getattr(getattr(env, "unwrapped", env), "step_dt", None)
            fps = 1.0 / dt if dt else 30.0
        self.frames_per_sec = float(fps)
        self.step_id = 0
        self.episode_id = -1
        self.recording = False
        self.recorded_frames: list = []
        self._video_name = None
        self.written: list[str] = []  # paths of the files written so far

    # ------------------------------------------------------------------ forwarding
    def __getattr__(self, name):
        if name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        return self.env.unwrapped

    # ------------------------------------------------------------------ recording
    def _capture_frame(self):
        frame = self.env.render()
        if frame is None:
            raise RuntimeError("RecordVideo: env.render() returned None")
        self.recorded_frames.append(frame.copy())
        if self.video_length and len(self.recorded_frames) >= self.video_length:
            self.stop_recording()

    def start_recording(self, video_name: str):
        if self.recording:
            self.stop_recording()
        self.recording = True
        self._video_name = video_name

    def stop_recording(self):
        if self.recording and self.recorded_frames:
            from PIL import Image

            path = os.path.join(self.video_folder, self._video_name + VIDEO_FORMATS[self.video_format])
            imgs = [Image.fromarray(f) for f in self.recorded_frames]
            kw = dict(save_all=True, append_images=imgs[1:], duration=1000.0 / self.frames_per_sec, loop=0)
            if self.video_format == "gif":
                imgs[0].save(path, format="GIF", **kw)
            else:
                imgs[0].save(path, format="PNG", default_image=False, **kw)
            self.written.append(path)
            if not self.disable_logger:
                print(f"[RecordVideo] wrote {path} ({len(imgs)} frames)")
        self.recorded_frames = []
        self.recording = False
        self._video_name = None

    def _video_enabled(self) -> bool:
        if self.step_trigger is not None:
            return bool(self.step_trigger(self.step_id))
        return bool(self.episode_trigger(self.episode_id))

    def reset(self, *args, **kwargs):
        out = self.env.reset(*args, **kwargs)
        self.episode_id += 1
        if self.recording and not self.video_length:
            self.stop_recording()
        if not self.recording and self._video_enabled():
            self.start_recording(self._name())
        if self.recording:
            self._capture_frame()
        return out

    def step(self, action):
        out = self.env.step(action)
        self.step_id += 1
        if not self.recording and self._video_enabled():
            self.start_recording(self._name())
        if self.recording:
            self._capture_frame()
        return out

    def _name(self) -> str:
        if self.step_trigger is not None:
            return f"{self.name_prefix}-step-{self.step_id}"
        return f"{self.name_prefix}-episode-{self.episode_id}"

    def render(self):
        return self.env.render()

    def close(self):
        if self.recording:
            self.stop_recording()
        return self.env.close()
