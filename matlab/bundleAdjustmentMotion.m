function [refinedPose, reprojectionErrors] = bundleAdjustmentMotion(xyzPoints, imagePoints, absolutePose, intrinsics, varargin)
%BUNDLEADJUSTMENTMOTION libvo (MI355X) shadow: motion-only bundle adjustment of one camera pose.
%   [refinedPose, reprojectionErrors] = bundleAdjustmentMotion(xyzPoints, imagePoints, ...
%       absolutePose, intrinsics, 'MaxIterations', 20, 'AbsoluteTolerance', 0, ...
%       'RelativeTolerance', 1e-9, 'PointsUndistorted', true)
%   the call the toolbox's stereo visual-odometry recipe makes right after
%   estworldpose (VO.m:123-130 uses estworldpose's pose as it is): least squares
%   on the pixel reprojection error over the given points, the points held
%   fixed, from absolutePose (rigidtform3d, camera pose in the world).  Pass the
%   inliers only: xyzPoints(inlierIdx, :), imagePoints(inlierIdx, :).
%   AbsoluteTolerance is in squared pixels per point.
%   libvo models no lens distortion here: PointsUndistorted must be true, or
%   the intrinsics without distortion coefficients.
%   reprojectionErrors: M x 1 double, each point's pixel distance at refinedPose.
    p = inputParser;
    p.addParameter('MaxIterations', 20);
    p.addParameter('AbsoluteTolerance', 0);
    p.addParameter('RelativeTolerance', 1e-9);
    p.addParameter('PointsUndistorted', false);
    p.parse(varargin{:});
    if isobject(imagePoints), imagePoints = imagePoints.Location; end
    distorted = false;
    if isprop(intrinsics, 'RadialDistortion'), distorted = distorted || any(intrinsics.RadialDistortion ~= 0); end
    if isprop(intrinsics, 'TangentialDistortion'), distorted = distorted || any(intrinsics.TangentialDistortion ~= 0); end
    if distorted && ~p.Results.PointsUndistorted
        error('vo:bundleAdjustmentMotion:options', ...
              'bundleAdjustmentMotion: libvo takes undistorted points: undistort them and pass PointsUndistorted = true');
    end
    opts = double([p.Results.MaxIterations, p.Results.AbsoluteTolerance, p.Results.RelativeTolerance]);
    A0 = double(absolutePose.A);
    if nargout > 1
        [A, reprojectionErrors] = vo_mex('refinepose', double(xyzPoints), double(imagePoints), A0, double(intrinsics.K), opts);
    else
        A = vo_mex('refinepose', double(xyzPoints), double(imagePoints), A0, double(intrinsics.K), opts);
    end
    refinedPose = rigidtform3d(A);
end
