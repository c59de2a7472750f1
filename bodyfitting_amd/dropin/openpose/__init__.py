"""`openpose` of the reference (openpose/body.py, openpose/hand.py, openpose/util.py, openpose/infer_openpose.py) on the HIP path:
`from openpose.body import Body` and `from openpose.hand import Hand` resolve here when bodyfitting_amd/dropin is on sys.path.
util's drawing functions return the canvas unchanged (said once on stderr)."""
