function [J, newOrigin] = undistortImage(I, intrinsics, varargin)
%UNDISTORTIMAGE libvo (MI355X) shadow: J = undistortImage(I, intrinsics)
%   reference call sites: VO.m:75-76.  intrinsics is a cameraIntrinsics object
%   or a struct with FocalLength, PrincipalPoint, Skew, RadialDistortion (2 or
%   3 entries) and TangentialDistortion.  Brown-Conrady remap on the device:
%   bilinear, OutputView 'same', FillValues 0; an interpolation argument and
%   name-value options are accepted only at these defaults, anything else
%   raises vo:undistortImage:options (the gateway parses them).  The uint8
%   image is handed over as it lies (column-major); the gateway passes
%   PrincipalPoint - 1, libvo's 0-based pixel indices.  Zero distortion (VO.m:50-51)
%   returns I without a call into libvo.
    k = double(intrinsics.RadialDistortion(:).');
    p = double(intrinsics.TangentialDistortion(:).');
    newOrigin = [0 0];
    if ~any(k) && ~any(p) && isempty(varargin)
        J = I;
        return
    end
    if numel(k) < 3
        k(3) = 0;
    end
    skew = 0;
    if isprop(intrinsics, 'Skew') || isfield(intrinsics, 'Skew')
        skew = double(intrinsics.Skew);
    end
    cam = [double(intrinsics.FocalLength(:).'), double(intrinsics.PrincipalPoint(:).'), skew, k, p];
    J = vo_mex('undistort', I, cam, varargin{:});
end
