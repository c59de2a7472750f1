"""`openpose` of the reference (openpose/body.py, openpose/infer_openpose.py) on the HIP path: `from openpose.body import Body`
resolves here when bodyfitting_amd/dropin is on sys.path.  Hands (openpose/hand.py) and drawing are not provided."""
