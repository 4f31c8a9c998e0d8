// The persistent build pipeline (round 4: the build loop of a chunk as resident kernels handing windows to each other through
// device-side queues) was measured at 24.9 k windows/s against 30.5 k for the lock-step plan and removed.  Its record: DESIGN.md
// section 10, profiles/r4_pipeline_*, and this file's git history.  Nothing includes this file.
